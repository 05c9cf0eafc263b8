"""Compare two gfx950 assembly listings of one translation unit (hipcc --cuda-device-only -S), kernel by kernel -- the code-generation evidence of a
refactor that moves text (profiles/attention_blocks_refactor.txt):  python tools/asm_kernel_counts.py PARENT.s NEW.s [name-substring ...]
Kernels whose name holds one of the substrings are reported with their registers, spills, scratch and the counts of v_mfma, LDS-DMA, ds_read_b128,
s_barrier and s_waitcnt vmcnt(n) per n; every other kernel must be the same text after normalising local labels.  Exit status 1 on a mismatch."""
import collections
import re
import sys


def kernels(path):
    text = open(path).read()
    meta = {}
    for m in re.finditer(r"  - \.agpr_count:.*?\n(?=  - \.agpr_count:|amdhsa\.target|\.\.\.)", text, re.S):
        f = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)$", m.group(0), re.M))
        meta[f["name"]] = {"vgpr": int(f["vgpr_count"]), "vspill": int(f["vgpr_spill_count"]), "sspill": int(f["sgpr_spill_count"]),
                           "scratch": int(f["private_segment_fixed_size"])}
    out = {}
    for m in re.finditer(r"^(\w+):\s+; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if name not in meta:
            continue
        lines = [ln if "#ASM" in ln else re.sub(r"\s*;.*", "", ln) for ln in body.splitlines()]
        c = collections.Counter()
        in_asm = False
        for ln in lines:
            in_asm = (in_asm or "#ASMSTART" in ln) and "#ASMEND" not in ln
            c["ds_read_b128_asm"] += in_asm and "ds_read_b128" in ln  # written out in inline asm: the K loops' fragment reads (the epilogues' scratch reads are the compiler's)
            c["mfma"] += "v_mfma" in ln
            c["ldsdma"] += bool(re.search(r"\bbuffer_load_dword\w* .* lds$|global_load_lds_", ln))
            c["ds_read_b128"] += "ds_read_b128" in ln
            c["barrier"] += "s_barrier" in ln
            for n in re.findall(r"vmcnt\((\d+)\)", ln):
                c["vm" + n] += 1
        norm = re.sub(r"\.L\w+", ".L", "\n".join(lines))
        out[name] = (dict(meta[name], **{k: v for k, v in c.items() if v}), norm)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    watched = sys.argv[3:]
    bad = same = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"  only in the {'parent' if name in a else 'new tree'}: {name}")
            bad += 1
        elif any(w in name for w in watched):
            (ca, ta), (cb, tb) = a[name], b[name]
            diff = sorted(k for k in set(ca) | set(cb) if ca.get(k, 0) != cb.get(k, 0))
            must = [k for k in diff if k not in ("vgpr", "sspill")]
            bad += bool(must) or cb["vgpr"] > ca["vgpr"]
            print(f"  {name}\n     text {'identical' if ta == tb else 'differs'}; {'differs in ' + ','.join(diff) if diff else 'all counts equal'}")
            fmt = lambda c: " ".join(f"{k}={c[k]}" for k in sorted(c, key=lambda k: (k[:2] == "vm", len(k), k)))
            print(f"     parent: {fmt(ca)}\n     new:    {fmt(cb)}")
        elif a[name][1] != b[name][1]:
            print(f"  {name}: text differs OUTSIDE the watched kernels")
            bad += 1
        else:
            same += 1
    print(f"  every other kernel: {same} byte-identical after label normalisation")
    print("RESULT:", "MISMATCH" if bad else "counts equal, no VGPR count above the parent's")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
