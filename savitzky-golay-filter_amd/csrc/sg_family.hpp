// sg_family.hpp -- names of a 16-bit storage family's own symbols.  The instantiation files of the 16-bit-storage kernels (sg_k1d_st16.hip,
// sg_k1d_st16_momenth.hip, sg_k1d_multi_st16.hip, sg_stream_dma_st16.hip, sg_stream_dma_multi_st16.hip) are compiled once per family,
// -DSG_FAMILY=h16|i16: SG_FAMILY_NAME(sg1d_, _kernel) is that family's sg1d_h16_kernel / sg1d_i16_kernel.
#pragma once

#ifdef SG_FAMILY
#define SG_CAT3_(a, b, c) a##b##c
#define SG_CAT3(a, b, c) SG_CAT3_(a, b, c)
#define SG_FAMILY_NAME(pre, post) SG_CAT3(pre, SG_FAMILY, post)
#endif
