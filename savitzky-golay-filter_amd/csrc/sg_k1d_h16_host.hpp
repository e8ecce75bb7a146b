// sg_k1d_h16_host.hpp -- JobH16 and the launchers of its objects live in sg_k1d_st16_host.hpp, with the other 16-bit-storage jobs; this name stays for
// the sources that include it.
#pragma once

#include "sg_k1d_st16_host.hpp"
