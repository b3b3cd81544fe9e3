"""Compare the kernels of two gfx950 assembly files (hipcc --cuda-device-only -S) of the same source before and after a
change that should not move the code: one line per kernel with the descriptor fields that set residency (VGPRs, the
AGPR offset, scratch, LDS), the instruction counts, the number of differing mnemonics over the whole kernel and over
the main loop (first to last MFMA), and the size of the mnemonic multiset difference over the whole kernel (0 with a
non-zero "whole": the same instructions in another order; otherwise instructions were added, dropped or exchanged).
Mnemonics only: register numbers, offsets and labels may differ. With a name filter, a second line per kernel gives
the ds_read_b128 count of every span between two consecutive s_barrier, in text order, from the kernel's first
barrier to the first one behind its last MFMA (the K loop of the GEMM kernels), old -> new.

Exit status 1 if the kernel sets differ, a descriptor field differs, or the MFMA-span mnemonic sequence differs.

usage: python tools/kdiff.py <old.s> <new.s> [name-filter-regex]
"""
import collections
import difflib
import re
import subprocess
import sys

FIELDS = ("next_free_vgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    """{symbol: (descriptor fields, [mnemonic, ...])}"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        name, desc = m.group(1), m.group(2)
        field = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", desc)}
        body = re.search(r"^" + re.escape(name) + r":(.*?)\.Lfunc_end", text, re.S | re.M).group(1)
        ops = [ln.split()[0] for ln in map(str.strip, body.splitlines())
               if ln and ln[0] not in ".;" and not ln.split()[0].endswith(":")]
        out[name] = ({k: field.get(k, 0) for k in FIELDS}, ops)
    return out


def mfma_span(ops):
    at = [i for i, op in enumerate(ops) if op.startswith("v_mfma")]
    return ops[at[0]:at[-1] + 1] if at else []


def reads_per_span(ops):
    bars = [i for i, op in enumerate(ops) if op == "s_barrier"]
    at = [i for i, op in enumerate(ops) if op.startswith("v_mfma")]
    if not bars or not at or bars[-1] < at[-1]:
        return []
    end = min(b for b in bars if b > at[-1])
    cut = [b for b in bars if b <= end]
    return [ops[a:b].count("ds_read_b128") for a, b in zip(cut, cut[1:])]


def ndiff(a, b):
    """mnemonics of either sequence outside their longest common alignment"""
    if a == b:
        return 0, []
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    n, what = 0, []
    for tag, i1, i2, j1, j2 in sm.get_opcodes():
        if tag != "equal":
            n += max(i2 - i1, j2 - j1)
            what += [f"-{op}" for op in a[i1:i2]] + [f"+{op}" for op in b[j1:j2]]
    return n, what


def msdiff(a, b):
    """size of the mnemonic multiset difference: 0 when one sequence is a reordering of the other"""
    ca, cb = collections.Counter(a), collections.Counter(b)
    return sum(((ca - cb) + (cb - ca)).values())


def demangle(names):
    for tool in ("c++filt", "llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt"):
        try:
            r = subprocess.run([tool, *names], capture_output=True, text=True, check=True)
            return dict(zip(names, r.stdout.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            pass
    return {n: n for n in names}


def main(argv):
    old, new = kernels(argv[1]), kernels(argv[2])
    flt = re.compile(argv[3]) if len(argv) > 3 else None
    bad = 0
    for n in sorted(set(old) ^ set(new)):
        print(f"ONLY IN {'old' if n in old else 'new'}: {n}")
        bad = 1
    both = sorted(set(old) & set(new))
    pretty = demangle(both)
    for n in both:
        short = re.sub(r"^void |\(anonymous namespace\)::", "", pretty[n]).split("(")[0]
        if flt and not flt.search(short):
            continue
        (fo, oo), (fn, on) = old[n], new[n]
        desc = " ".join(f"{k.split('_')[0]}={fo[k]}" + ("" if fo[k] == fn[k] else f"->{fn[k]} DIFF") for k in FIELDS)
        whole, what = ndiff(oo, on)
        span, _ = ndiff(mfma_span(oo), mfma_span(on))
        if fo != fn or span:
            bad = 1
        print(f"{short:<52} {desc}  insts {len(oo)}->{len(on)}  diff whole {whole} mfma-span {span} multiset {msdiff(oo, on)}"
              + (f"  [{' '.join(what[:24])}{' ...' if len(what) > 24 else ''}]" if what else ""))
        if flt and reads_per_span(on):
            print(f"    ds_read_b128 per barrier span: {reads_per_span(oo)} -> {reads_per_span(on)}")
    print("FAIL" if bad else "OK", f"({len(both)} kernels)")
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv))
