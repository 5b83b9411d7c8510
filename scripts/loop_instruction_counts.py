"""Static instruction counts of one fused k_f build's trace loops, per segment of the loop (developer tool; the tables
of profiles/cx_products_instruction_counts.txt).

    python scripts/loop_instruction_counts.py [--cfg 109] [--csrc DIR] [--listing FILE.s] [extra hipcc flags, e.g. -DNAME]

Compiles csrc/kernels.hip for gfx950 with the flags of scripts/kernel_resources.py plus --cuda-device-only -S
-gline-tables-only (line tables only: the instructions are those of the build without them), takes
k_f<FPlan<16,16,8>, 2, CFG> out of the listing and prints one table for every loop of more than 1000 instructions that
lies in no other loop (the trace loops; the fast one, whose time multipliers sit in LDS, is the shorter).

Segments.  Every instruction carries the line of the innermost inlined function it came from (.loc).  Helpers (cx_mul_batch,
the butterflies, the splits) are shared by all segments, so an instruction belongs to the segment that the loop is in at
that point of the listing, and the segment changes where the first instruction of its anchor function appears:
f_spectrum_epilogue -> "spectrum epilogue", f_inverse_input -> "inverse input + pass 1", f_core_pass23 behind that ->
"passes 2-3", f_time_epilogue -> "time epilogue"; everything in front is "window + forward".  The scheduler moves
instructions a few slots across such a border (fences and barriers keep it to that), so the rows are good to a handful of
instructions and their sum is exact.  The listing holds the pruned and the full inverse input with a pass 1 each (a trace
runs one) and the epilogue's group body once (a trace runs it 8 times): one pass through the listing, not one trace."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SEGS = ["window + forward", "spectrum epilogue", "inverse input + pass 1", "passes 2-3", "time epilogue"]
COLS = ["VALU", "packed fp32", "v_xor flips", "v_mov v,v", "v_pk_add ..,0", "s_nop", "LDS"]


def classify(ins):
    op = ins.split()[0]
    c = []
    if op.startswith("v_") and op != "v_nop":
        c.append("VALU")
    if re.match(r"v_pk_(mul|fma|add)_f32", op):
        c.append("packed fp32")
    if op.startswith("v_xor_b32") and "0x80000000" in ins:
        c.append("v_xor flips")
    if re.match(r"v_mov_b32(_e32)?\s+v\d+,\s*v\d+\s*$", ins):
        c.append("v_mov v,v")
    if op == "v_pk_add_f32" and re.search(r",\s*0(\s|$)", ins):
        c.append("v_pk_add ..,0")
    if op == "s_nop":
        c.append("s_nop")
    if op.startswith("ds_"):
        c.append("LDS")
    return c


def function_ranges(header):
    """(first line, name) of every function definition of fft_f.hpp, in order"""
    out = []
    for n, line in enumerate(open(header), 1):
        m = re.match(r"(?:__device__|__global__|constexpr)\b[^;]*?\b(\w+)\(", line)
        if m:
            out.append((n, m.group(1)))
    return out


def main():
    args = sys.argv[1:]
    cfg, csrc, listing = 109, os.path.join(HERE, "..", "thz_image_explorer_amd", "csrc"), None
    for flag in ("--cfg", "--csrc", "--listing"):
        if flag in args:
            i = args.index(flag)
            v = args[i + 1]
            del args[i:i + 2]
            if flag == "--cfg":
                cfg = int(v)
            elif flag == "--csrc":
                csrc = v
            else:
                listing = v
    if listing is None:
        listing = os.path.join(tempfile.mkdtemp(), "kernels.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                        "-gline-tables-only", "kernels.hip", "-o", listing] + args, cwd=csrc, check=True)
    funcs = function_ranges(os.path.join(csrc, "fft_f.hpp"))

    def func_at(line):
        name = None
        for first, f in funcs:
            if first > line:
                break
            name = f
        return name

    want = re.compile(r"^_ZN3thz3k_fINS_5FPlanILi16ELi16ELi8EEELi2ELi%dEEEv.*:\s*(;.*)?$" % cfg)
    body, inside, hdr_file = [], False, None
    for line in open(listing):
        m = re.match(r'\s*\.file\s+(\d+)\s+.*"fft_f\.hpp"', line)
        if m:
            hdr_file = m.group(1)
        if not inside:
            inside = bool(want.match(line))
            continue
        if line.startswith(".Lfunc_end"):
            break
        body.append(line.rstrip("\n"))
    assert body, "kernel not found in the listing"
    # instructions with the function of their .loc line, labels with their position
    ins, labels, fn = [], {}, None
    for line in body:
        t = line.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            fn = func_at(int(m.group(2))) if m.group(1) == hdr_file else None
            continue
        m = re.match(r"(\.LBB\d+_\d+):", t)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if not t or t.startswith((".", ";")) or t.endswith(":"):
            continue
        ins.append((t.split(";")[0].strip(), fn))
    loops = []
    for i, (t, _) in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", t)
        if m and m.group(1) in labels and labels[m.group(1)] <= i:
            loops.append((labels[m.group(1)], i))
    outer = [l for l in loops if l[1] - l[0] > 1000 and not any(o != l and o[0] <= l[0] and l[1] <= o[1] for o in loops)]
    for lo, hi in sorted(outer):
        seg, rows, switches = 0, {s: dict.fromkeys(COLS, 0) for s in SEGS}, []
        for k in range(lo, hi + 1):
            t, f = ins[k]
            new = seg
            if f == "f_spectrum_epilogue" and seg < 1:
                new = 1
            elif f == "f_inverse_input" and seg != 2:
                new = 2
            elif f == "f_core_pass23" and seg == 2:
                new = 3
            elif f == "f_time_epilogue" and seg in (2, 3):
                new = 4
            if new != seg:
                seg = new
                switches.append(f"{SEGS[seg]} at +{k - lo}")
            for c in classify(t):
                rows[SEGS[seg]][c] += 1
        print(f"loop of {hi - lo + 1} instructions, k_f<FPlan<16,16,8>, 2, {cfg}>   ({'; '.join(switches)})")
        print(f"{'segment':26s}" + "".join(f"{c:>15s}" for c in COLS))
        for s in SEGS:
            print(f"{s:26s}" + "".join(f"{rows[s][c]:15d}" for c in COLS))
        print(f"{'whole loop':26s}" + "".join(f"{sum(rows[s][c] for s in SEGS):15d}" for c in COLS))
        print()


if __name__ == "__main__":
    main()
