"""Per-kernel comparison of the gfx950 code in two builds of a library (or two objects):
   python tools/isa_diff.py LIB_A LIB_B > profiles/some_isa_diff.txt
Whole code objects never compare equal (a symbol follows the source text), so every kernel is disassembled on its own, addresses and branch
targets are normalised (a kernel that merely moved reads as the same; so does one that is no longer, or newly, the last of its code object and lost or
gained the object's end padding), and each name prints `same` or `differs`; for those that differ the
VGPRs, SGPRs, LDS bytes, scratch (private segment) bytes and code length of both sides follow."""
import os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import READELF, code_objects
from kernel_isa import OBJDUMP


def tool(cmd, blob):
    with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
        f.write(blob)
    txt = subprocess.run(cmd + [f.name], capture_output=True, text=True).stdout
    os.unlink(f.name)
    return txt


def kernels(path):
    """demangled kernel name -> (normalised instruction list, resources)"""
    out = {}
    for co in code_objects(open(path, "rb").read()):
        res = {}
        for block in tool([READELF, "--notes"], co).split("- .agpr_count:")[1:]:
            g = lambda key: int(re.search(r"\." + key + r":\s+(\S+)", block).group(1))
            res[re.search(r"\.name:\s+(\S+)", block).group(1)] = {"vgpr": g("vgpr_count"), "sgpr": g("sgpr_count"), "lds": g("group_segment_fixed_size"),
                                                                  "scratch": g("private_segment_fixed_size")}
        # kernels are matched by their mangled names (llvm-objdump --demangle and c++filt spell vector types differently) and printed demangled
        pretty = dict(zip(res, subprocess.run(["c++filt"] + list(res), capture_output=True, text=True).stdout.split("\n"))) if res else {}
        found = set()
        for block in re.split(r"\n(?=[0-9a-f]{16} <)", tool([OBJDUMP, "-d"], co)):
            head, _, body = block.partition("\n")
            m = re.match(r"([0-9a-f]{16}) <(.*)>:$", head)
            if not m or m.group(2) not in res:
                continue
            start, ins, at = int(m.group(1), 16), [], []
            for line in body.split("\n"):
                # "\ts_cbranch_scc1 65500   // 000000001234: BF85FFDC <name+0x1c>": keep the mnemonic and operands; a branch keeps its target's offset
                # inside the kernel instead of the encoded distance (which is the same thing, but the encoding column goes)
                t = re.match(r"\s+(\S+)(.*?)\s*// ([0-9A-F]{12}): [0-9A-F ]+(?:<.*?\+0x([0-9a-f]+)>)?", line)
                if t:
                    ins.append(t.group(1) + ((" @" + t.group(4)) if t.group(4) and t.group(1).startswith("s_") else t.group(2)))
                    at.append(int(t.group(3), 16))
            # the s_nop run that pads the end of a code object is listed under its LAST kernel: not that kernel's code (no kernel ends in an s_nop it runs),
            # and which kernel is last changes when two translation units become one
            while ins and ins[-1].startswith("s_nop"):
                ins.pop(), at.pop()
            end = at[-1] if ins else start
            out[re.sub(r"\(.*", "", pretty[m.group(2)])] = (ins, dict(res[m.group(2)], code=end - start + 4))
            found.add(m.group(2))
        assert found == set(res), f"kernels in the metadata that the disassembly does not show: {sorted(set(res) - found)[:3]}"
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    same = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"only in {'A' if name in a else 'B'}  {name}")
        elif a[name][0] == b[name][0] and a[name][1] == b[name][1]:
            same += 1
            print(f"same     {name}")
        else:
            print(f"differs  {name}")
            for side, (_, r) in (("A", a[name]), ("B", b[name])):
                print(f"         {side}: vgpr {r['vgpr']:>3} sgpr {r['sgpr']:>3} lds {r['lds']:>6} scratch {r['scratch']:>3} code {r['code']:>6}")
    print(f"# {same} same, {len(set(a) | set(b)) - same} differ or are missing on one side; A = {sys.argv[1]}, B = {sys.argv[2]}")


if __name__ == "__main__":
    main()
