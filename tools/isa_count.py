"""Static VALU count of one kernel from hipcc's assembly listing, per loop depth and per inner loop, weighted by the issue-cost table of
profiles/r02_ubench_issue.txt (two waves per SIMD).  No GPU needed:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form --cuda-device-only -S \
          -o spd_pairwise.s gabotorch_amd/csrc/spd_pairwise.hip
    python tools/isa_count.py spd_pairwise.s spd_ai_pairwise_kernelILi10E

For spd_ai_pairwise_kernel<D>: depth 1 is the row loop (congruence, tridiagonalisation, order flip, trailing 2x2, logarithms, exp - executed once per
pair), each depth-2 loop is one QL stage (executed once per sweep: sweep control + the stage's unrolled steps).
"""
import collections
import re
import sys

# cycles per instruction per SIMD at two waves (profiles/r02_ubench_issue.txt); 32-bit VALU: the v_fma_f32 row
CYCLES = {"fma64": 4.5, "cmp64": 6.0, "trans64": 13.66, "cndmask": 3.65, "mov64": 4.25, "ldexp64": 5.13, "frexp64": 4.67, "valu32": 3.75}


def classify(op):
    if op.startswith(("v_rcp_f64", "v_rsq_f64", "v_sqrt_f64")):
        return "trans64"
    if op.startswith("v_cmp") and "f64" in op:
        return "cmp64"
    if op.startswith("v_cndmask"):
        return "cndmask"
    if op.startswith(("v_mov_b64", "v_lshl_add_u64")):
        return "mov64"
    if op.startswith("v_ldexp_f64"):
        return "ldexp64"
    if op.startswith("v_frexp"):
        return "frexp64"
    if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
        return None                                  # scalar-unit traffic, not a VALU issue slot of the lanes' arithmetic
    if "f64" in op:
        return "fma64"
    return "valu32"


def main():
    path, match = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(k for k, l in enumerate(lines) if l.startswith("_Z") and match in l.split(":")[0])
    end = next(k for k in range(start, len(lines)) if lines[k].strip().startswith("s_endpgm"))
    # hipcc annotates every basic-block label with its loop: "; in Loop: Header=BBx_y Depth=n" for a block inside a loop, "; =>This [Inner] Loop
    # Header: Depth=n" for a loop's own header (on the label's line, or on the line after a "Parent Loop ..." one), nothing outside loops
    depth, loop = 0, "-"
    per_depth = collections.defaultdict(collections.Counter)
    per_loop = collections.defaultdict(collections.Counter)
    for l in lines[start:end]:
        label = re.match(r"^(?:\.L|; %bb\.)(\w+):", l)
        continuation = not label and l[:1] in " \t" and l.strip().startswith(";") and "Loop" in l
        note = l[label.end():] if label else l
        if label or continuation:
            d = re.search(r"Depth=(\d+)", note)
            h = re.search(r"Header=(BB\d+_\d+)", note)
            if h:
                depth, loop = int(d.group(1)), h.group(1)
            elif "Loop Header" in note:
                depth = int(d.group(1))
                if label:
                    loop = label.group(1)
            elif "Parent Loop" in note and label:
                loop = label.group(1)                  # its own "This Inner Loop Header" line follows
            elif label:
                depth, loop = 0, "-"
            continue
        t = l.strip()
        if not t.startswith("v_"):
            continue
        cls = classify(t.split()[0])
        if cls is None:
            continue
        per_depth[depth][cls] += 1
        if depth >= 2:
            per_loop[loop][cls] += 1

    def show(name, cnt):
        n = sum(cnt.values())
        cyc = sum(CYCLES[k] * v for k, v in cnt.items())
        print(f"{name:>14}: {n:5d} VALU  {cyc:8.0f} cycles = {cyc / 4.5:7.1f} FMA slots   " + "  ".join(f"{k} {v}" for k, v in sorted(cnt.items())))

    for d in sorted(per_depth):
        show(f"depth {d}", per_depth[d])
    for name, cnt in per_loop.items():
        show(name, cnt)
        steps = cnt["trans64"] - 1         # one v_rcp_f64 per QL step + the shift's v_rsq_f64
        print(f"{'':>14}  sweep control = loop body minus {steps} steps x 16 VALU: {sum(cnt.values()) - 16 * steps} VALU")


if __name__ == "__main__":
    main()
