"""Instruction counts of one kernel's gfx950 ISA listing, cut at the workgroup barriers.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --save-temps -c plenoctree_amd/csrc/mlp_kernels.hip -o /tmp/mlp.o
    python scripts/isa_phases.py mlp_kernels-hip-amdgcn-amd-amdhsa-gfx950.s mlp_fwd_kernelILi2ELb1ELb1ELb1E

The fused MLP kernels are straight-line code between barriers apart from the k-loops, so "one row per barrier-to-barrier
stretch" is a phase table: vector ALU (MFMAs apart), MFMA, LDS reads / writes, vector-memory loads / stores and scalar
instructions per stretch, in program order.  A stretch that holds a backward branch is a loop; its label and the branch are
printed so that the body can be told from the code around it (the counts of such a stretch are those of ONE trip plus the
straight-line code before and after it inside the same stretch; `--loops` prints the loop bodies on their own).
The resource lines (.vgpr_count, scratch, code bytes) of the kernel's metadata are printed first.
"""
import argparse
import re
import sys

CLASSES = ("valu", "mfma", "lds_rd", "lds_wr", "vm_ld", "vm_st", "salu", "wait")


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds_rd" if ("read" in op or "load" in op or "bpermute" in op or "permute" in op or "swizzle" in op) else "lds_wr"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vm_st" if ("store" in op or "atomic" in op) else "vm_ld"
    if op in ("s_waitcnt", "s_nop", "s_barrier", "s_sleep"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return None


def kernel_body(lines, name):
    label = lambda ln: ln.split(";")[0].strip()
    start = next((i for i, ln in enumerate(lines) if ln.startswith("_Z") and name in label(ln) and label(ln).endswith(":")), None)
    if start is None:
        sys.exit(f"no kernel matching {name!r}")
    end = next(i for i in range(start, len(lines)) if lines[i].lstrip().startswith(".Lfunc_end"))
    return label(lines[start]).rstrip(":"), lines[start + 1:end]


def metadata(lines, symbol):
    out = {}
    keys = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
            "vgpr_spill_count", "sgpr_spill_count")
    hit = False
    block = []
    for ln in lines:
        s = ln.strip()
        if s.startswith("- .agpr_count") or s.startswith("- .args"):
            block = []
        block.append(s)
        if s.startswith(".name:") and s.split()[-1] == symbol:
            hit = True
        if hit and s.startswith(".wavefront_size"):
            break
        if s.startswith(".wavefront_size"):
            block = []
    for s in block:
        for k in keys:
            if s.lstrip("- ").startswith("." + k + ":"):
                out[k] = s.split()[-1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("kernel", help="substring of the mangled kernel name")
    ap.add_argument("--loops", action="store_true", help="also print every loop body (label .. backward branch) on its own")
    args = ap.parse_args()
    with open(args.listing) as f:
        lines = f.readlines()
    symbol, body = kernel_body(lines, args.kernel)
    print(symbol)
    print("  " + " ".join(f"{k}={v}" for k, v in metadata(lines, symbol).items()))

    label_at = {}
    insts = []           # (op, text)
    for ln in body:
        s = ln.split(";")[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.LBB\S+):", s)
            if m:
                label_at[m.group(1)] = len(insts)
            continue
        m = re.match(r"^(\.LBB\S+):", s)
        if m:
            label_at[m.group(1)] = len(insts)
            continue
        insts.append((s.split()[0], s))
    print(f"  instructions={len(insts)}")

    loops = []           # (first, last) instruction indices of label .. backward branch
    for i, (op, text) in enumerate(insts):
        if op.startswith("s_cbranch") or op == "s_branch":
            tgt = text.split()[-1]
            if tgt in label_at and label_at[tgt] <= i:
                loops.append((label_at[tgt], i, tgt))

    def count(lo, hi):
        c = dict.fromkeys(CLASSES, 0)
        for op, _ in insts[lo:hi]:
            k = classify(op)
            if k:
                c[k] += 1
        return c

    fmt = lambda c: " ".join(f"{k}={c[k]:<5d}" for k in CLASSES)
    cuts = [-1] + [i for i, (op, _) in enumerate(insts) if op == "s_barrier"] + [len(insts)]
    print("  stretch  insts        " + "  (loops inside: label, trips' body [first,last])")
    for n in range(len(cuts) - 1):
        lo, hi = cuts[n] + 1, cuts[n + 1]
        inside = [(a, b, t) for a, b, t in loops if lo <= b < hi or lo <= a < hi]
        mf = [i for i in range(lo, hi) if classify(insts[i][0]) == "mfma"]
        # vector-ALU instructions between the stretch's first and last MFMA: what the GEMM itself interleaves
        span = f"valu_between_mfmas={count(mf[0], mf[-1])['valu']:<4d}" if mf else " " * 23
        print(f"  {n:3d} [{lo:6d},{hi:6d})  {fmt(count(lo, hi))} {span} " + " ".join(f"{t}[{a},{b}]" for a, b, t in inside))
    if args.loops:
        print("  loop bodies")
        for a, b, t in loops:
            print(f"  {t:12s} [{a:6d},{b:6d}]  {fmt(count(a, b + 1))}")


if __name__ == "__main__":
    main()
