#!/usr/bin/env python3
"""Offline hunt for the Philox counters whose words drive the fixed fp32 functions of SPEC S2 to their extremes: the
source of the HUNTED table in tests/test_gpu_pf_exact.py (pasted there as data; tests/test_gpu_pf_exact.py's CPU test
recomputes every entry with oracle.pf.philox4x32_10 and classifies it again, so nothing trusts this file's Philox).

A vectorised numpy Philox4x32-10 sweeps counter (gi, frame, 0, c3) for one seed over gi < 2^12 and frames 1, 2, ...
(the frame is swept, not a wider index: SPEC S16's search predict needs gi < P <= 2^24, and a hit below 4099 lies inside
the exact tests' whole-batch runs at global_begin 0). Counter kinds and the words the predict kernels read of them:

  c3 = 0  walk    words 0, 2 -> ln (n0 / n1 and n2's radius), words 1, 3 -> sincos       (vpf_predict, _cv, _search)
  c3 = 1  cv      word 0 -> ln, word 1 -> sincos                                          (vpf_predict_cv)
  c3 = 2  angle   word 0 -> ln, word 1 -> sincos                                          (vpf_predict_angle)
  c3 = 3  search  words 0, 1 -> the lattice jitter u0, u1                                 (vpf_predict_search)

Classes of a word w, k = w >> 9 (23 bits), u = (2 k + 1) 2^-24:
  log_lo    k == 0: u = 2^-24, the largest radius sqrt(-2 ln u) = 5.77
  log_hi    k == 2^23 - 1: u = 1 - 2^-24, the smallest radius
  split_hi  2 k + 1 == 0xB504F3: fixed_logf's mantissa m is fp32(0.70710678) itself (the branch not taken)
  split_lo  2 k + 1 == 0x5A8279: m is the fp32 number just below it (the branch taken)
  ang_qN_lo k >> 21 == N and k mod 2^21 == 0: quadrant N of fixed_sincos2pi at r = 2^-22
  ang_qN_hi k >> 21 == N and k mod 2^21 == 2^21 - 1: quadrant N at r = 1 - 2^-22
  u_lo/u_hi the jitter at u = 2^-24 / 1 - 2^-24
  exp_cut   (c3 = 0, word 2) |n2| > 5.5: 16 n2 passes fixed_expf's 88 clamp and -16 n2 its exact zero below -87; found
            from k(word 2) <= 2 and an fp64 estimate of the cosine, which the CPU test confirms with the oracle

Each class has probability 2^-23 per word; the sweep stops at --frames and prints the first --keep hits of every
(c3, word, class) as rows (seed, frame, c2, c3, gi, word, class). 2^14 frames (2^26 counters per kind) take about
15 s per kind; exp_cut sweeps --exp-frames (default 2^15).

    python tools/philox_hunt.py --seed 1234 > table.txt
"""
import argparse
import sys

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
GI = 1 << 12
KINDS = {0: "walk", 1: "cv", 2: "angle", 3: "search"}
LOG_WORDS = {0: (0, 2), 1: (0,), 2: (0,), 3: ()}
ANG_WORDS = {0: (1, 3), 1: (1,), 2: (1,), 3: ()}
U_WORDS = {0: (), 1: (), 2: (), 3: (0, 1)}
K_MAX = (1 << 23) - 1
SPLIT_HI, SPLIT_LO = 0xB504F3, 0x5A8279


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (SPEC S1) of uint64 arrays holding 32-bit counters; four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in (c0, c1, c2, c3))
    for r in range(10):
        ka, kb = np.uint64((k0 + r * W0) & 0xFFFFFFFF), np.uint64((k1 + r * W1) & 0xFFFFFFFF)
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ ka, p1 & LO32, (p0 >> S32) ^ c3 ^ kb, p0 & LO32
    return c0, c1, c2, c3


def classes(c3, word, k):
    """{class: boolean mask} of the 23-bit values k of `word` of a counter of kind c3."""
    out = {}
    if word in LOG_WORDS[c3]:
        out.update(log_lo=k == 0, log_hi=k == K_MAX, split_hi=2 * k + 1 == SPLIT_HI, split_lo=2 * k + 1 == SPLIT_LO)
    if word in ANG_WORDS[c3]:
        low = k & ((1 << 21) - 1)
        for q in range(4):
            out[f"ang_q{q}_lo"] = (k >> 21 == q) & (low == 0)
            out[f"ang_q{q}_hi"] = (k >> 21 == q) & (low == (1 << 21) - 1)
    if word in U_WORDS[c3]:
        out.update(u_lo=k == 0, u_hi=k == K_MAX)
    return out


def sweep(seed, c3, frames, keep, found, exp_only=False, block=1 << 10):
    """Frames 1 .. frames of kind c3, `block` frames at a time; adds hits to found[(c3, word, class)] (frame-major)."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    gi = np.tile(np.arange(GI, dtype=np.uint64), block)
    for f0 in range(1, frames + 1, block):
        fr = np.repeat(np.arange(f0, f0 + block, dtype=np.uint64), GI)
        w = philox4x32_10(gi, fr, np.zeros_like(gi), np.full_like(gi, c3), k0, k1)
        ks = [(x >> np.uint64(9)).astype(np.int64) for x in w]
        if c3 == 0:
            cand = np.nonzero(ks[2] <= 2)[0]
            u2 = (2.0 * ks[2][cand] + 1.0) * 2.0 ** -24
            u3 = (2.0 * ks[3][cand] + 1.0) * 2.0 ** -24
            n2 = np.sqrt(-2.0 * np.log(u2)) * np.cos(2.0 * np.pi * u3)
            for i in cand[np.abs(n2) > 5.5005]:
                found.setdefault((0, 2, "exp_cut"), []).append((int(fr[i]), int(gi[i])))
        if exp_only:
            continue
        for word in range(4):
            for name, mask in classes(c3, word, ks[word]).items():
                for i in np.nonzero(mask)[0]:
                    found.setdefault((c3, word, name), []).append((int(fr[i]), int(gi[i])))
        print(f"# {KINDS[c3]}: frames {f0}..{f0 + block - 1} done", file=sys.stderr)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--frames", type=int, default=1 << 14)
    ap.add_argument("--exp-frames", type=int, default=1 << 15)
    ap.add_argument("--keep", type=int, default=2)
    a = ap.parse_args()
    found = {}
    for c3 in KINDS:
        sweep(a.seed, c3, a.frames, a.keep, found)
    if a.exp_frames > a.frames:
        rest = {}
        sweep(a.seed, 0, a.exp_frames, a.keep, rest, exp_only=True)
        found[(0, 2, "exp_cut")] = sorted(set(rest.get((0, 2, "exp_cut"), [])))
    print("# (seed, frame, c2, c3, gi, word, class)")
    for (c3, word, name) in sorted(found):
        for frame, gi in found[(c3, word, name)][:a.keep]:
            print(f"    ({a.seed}, {frame}, 0, {c3}, {gi}, {word}, \"{name}\"),")
    for c3 in KINDS:
        for word in range(4):
            for name in classes(c3, word, np.zeros(1, np.int64)):
                n = len(found.get((c3, word, name), []))
                if n < a.keep:
                    print(f"# {KINDS[c3]} word {word} {name}: only {n} hit(s); sweep more frames", file=sys.stderr)


if __name__ == "__main__":
    main()
