"""Same-process A/B of one C-ABI entry point between two builds of the library (design aid, GPU box only): the product
libvpf.so (bound by vitparticlefiltertracker_amd._lib) and another build loaded side by side with RTLD_LOCAL (default:
the lab build, tools/gemm_lab -> libvpf_lab.so, whose MX8 GEMM / attention are the round-3 snapshots). Both get the
same device buffers; interleaved rounds, HIP-event medians, outputs compared bit for bit.

Cases: bf16_qkv / bf16_proj / bf16_fc1 / bf16_fc2 (vpf_gemm_bf16 with the encoder's epilogues), mx8_fc1 (LN + GELU, MX8-only output: FC2's A operand), mx8_fc2 / mx8_proj (residual + planes + the MX8 copy of h),
mx8_qkv (LN fold, bf16 out), quant (vpf_quantize_mx8 of a bf16 [M][768] tensor), attn (bf16 attention, N = 197),
attn577 (bf16 attention at ViT-L/14 @ 336's N = 577, 16 heads), attn_mx8 (vpf_attention_bf16_mx8, N = 197, 12 heads: the
fp8 bytes and the scale bytes), crop / crop_rot (vpf_crop_patches_bf16 / _rot_bf16) and color / color_surround (vpf_color_weight / _surround) on AB_P
particles, attn_edges (bits only, no timing: every N of tests/test_oracle_attention.py's PIPE_N +
STREAM_N at B = H = 3 with q_rows = N and, at N = 197 / 400 / 577, one partial q_rows, then the MX8 output over Q8_N.
The MX8 part departs from B = H = 3: it runs at B = 3, H = 4, because vpf_attention_bf16_mx8 needs D = 64 H to be a
multiple of 128, which H = 3 is not (the tests make the same choice). Inputs randn * 1.5 with the planted key rows of
test_attention_bf16_rescale_branch, so the rescale and redo branches are compared too).

usage: python tools/lib_ab.py [rounds] [cases] [other_lib]      env AB_M (rows, default 4096*197),
                                                                AB_P (particles of the crop / colour cases, default 4096),
                                                                AB_PARTS (bf16 LN statistics planes, default K/64; 0 = {mean, rstd})
"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vitparticlefiltertracker_amd import _lib as E  # noqa: E402
from vitparticlefiltertracker_amd import ops  # noqa: E402,F401

V = torch.ops.vpf

# tests/test_oracle_attention.py's sizes: every path of the key-pipelined / key-streamed kernels and of the MX8 output
PIPE_N = [1, 8, 9, 16, 17, 33, 40, 41, 50, 192, 193, 197, 201, 209, 224, 256]
STREAM_N = [257, 264, 265, 272, 273, 288, 300, 330, 384, 400, 545, 577, 640]
Q8_N = [1, 33, 197, 256]
EDGE_PARTIAL_ROWS = {197: 100, 400: 385, 577: 300}


def attn_edges(P, O, pt, st, g, dev):
    """The attention entry points of both libraries over the edge sizes, bit for bit. Returns (runs, mismatches)."""
    def inputs(B, N, H):
        D = 64 * H
        qkv = (torch.randn(B, N, 3 * D, device=dev, generator=g) * 1.5).to(torch.bfloat16)
        for b in range(B):   # key rows aligned with query 5: far past the rescale threshold, below it, in the tail tile
            h = b % H
            q = qkv[b, min(5, N - 1), h * 64:(h + 1) * 64].float()
            for row, f in ((150, 12.0), (40, 1.5), (N - 1, 20.0)):
                if row < N:
                    qkv[b, row, D + h * 64:D + (h + 1) * 64] = (q * f).to(torch.bfloat16)
        return qkv
    runs, bad = 0, []
    B = H = 3
    for N in PIPE_N + STREAM_N:
        qkv = inputs(B, N, H)
        for q_rows in [N] + ([EDGE_PARTIAL_ROWS[N]] if N in EDGE_PARTIAL_ROWS else []):
            outs = [torch.zeros(B, N, 64 * H, device=dev, dtype=torch.bfloat16) for _ in range(2)]
            for L, o in zip((P, O), outs):
                assert L.vpf_attention_bf16(pt(qkv), pt(o), B, N, H, 64, 0.125, q_rows, st) == 0, (N, q_rows)
            torch.cuda.synchronize()
            runs += 1
            if not torch.equal(*outs):
                bad.append(("bf16", N, q_rows))
    H = 4   # not the H = 3 of the bf16 part: the MX8 output needs D = 64 H to be a multiple of 128
    for N in Q8_N:
        qkv = inputs(B, N, H)
        outs = [ops.mx8_empty(B * N, 64 * H, dev) for _ in range(2)]
        for L, (q8, s8) in zip((P, O), outs):
            q8.zero_()
            s8.zero_()
            assert L.vpf_attention_bf16_mx8(pt(qkv), B, N, H, 64, 0.125, pt(q8), q8.stride(0), pt(s8), s8.shape[1],
                                            st) == 0, N
        torch.cuda.synchronize()
        runs += 1
        if not (torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])):
            bad.append(("mx8", N, N))
    return runs, bad


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    cases = sys.argv[2].split(",") if len(sys.argv) > 2 else ["mx8_fc1", "mx8_fc2", "mx8_qkv", "quant", "attn"]
    other = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "vitparticlefiltertracker_amd", "libvpf_lab.so")
    P = E.lib()
    O = ctypes.CDLL(other, mode=ctypes.RTLD_LOCAL)
    for L in (P, O):
        L.vpf_gemm_mx8.argtypes = E.SIGNATURES["vpf_gemm_mx8"]
        L.vpf_quantize_mx8.argtypes = E.SIGNATURES["vpf_quantize_mx8"]
        L.vpf_attention_bf16.argtypes = E.SIGNATURES["vpf_attention_bf16"]
        L.vpf_attention_bf16_mx8.argtypes = E.SIGNATURES["vpf_attention_bf16_mx8"]
        L.vpf_gemm_bf16.argtypes = E.SIGNATURES["vpf_gemm_bf16"]
        for name in ("vpf_crop_patches_bf16", "vpf_crop_patches_rot_bf16", "vpf_color_weight",
                     "vpf_color_weight_surround"):
            getattr(L, name).argtypes = E.SIGNATURES[name]
    M = int(os.environ.get("AB_M", 4096 * 197))
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    pt = E.ptr
    for case in cases:
        outs = {}
        size = f"M={M}"
        if case == "attn_edges":
            runs, bad = attn_edges(P, O, pt, st, g, dev)
            for b in bad:
                print(f"{case:8s} differs: {b[0]} N={b[1]} q_rows={b[2]}", flush=True)
            print(f"{case:8s} {runs} runs  outputs bit-identical: {not bad}", flush=True)
            continue
        if case in ("attn", "attn577"):
            # attn: ViT-B/16 @ 224 (N = 197, 12 heads, the key-pipelined kernel); attn577: ViT-L/14 @ 336 (N = 577,
            # 16 heads, the key-streamed kernel), 4096 particles unless AB_M says otherwise
            N, H = (197, 12) if case == "attn" else (577, 16)
            B = M // 197
            qkv = (torch.randn(B, N, 3 * 64 * H, device=dev, generator=g) * 1.5).to(torch.bfloat16)
            bufs = {k: torch.empty(B, N, 64 * H, device=dev, dtype=torch.bfloat16) for k in ("product", "other")}

            def call(L, k):
                return L.vpf_attention_bf16(pt(qkv), pt(bufs[k]), B, N, H, 64, 0.125, N, st)
            flop = 4.0 * B * H * N * N * 64
        elif case == "attn_mx8":
            # the fp8 path's attention (MX8 output, the proj A operand): N = 197, 12 heads, timed like attn
            N, H = 197, 12
            B = M // 197
            qkv = (torch.randn(B, N, 3 * 64 * H, device=dev, generator=g) * 1.5).to(torch.bfloat16)
            bufs = {k: tuple(t.zero_() for t in ops.mx8_empty(B * N, 64 * H, dev)) for k in ("product", "other")}

            def call(L, k):
                q8, s8 = bufs[k]
                return L.vpf_attention_bf16_mx8(pt(qkv), B, N, H, 64, 0.125, pt(q8), q8.stride(0), pt(s8), s8.shape[1],
                                                st)
            flop = 4.0 * B * H * N * N * 64
        elif case in ("crop", "crop_rot", "color", "color_surround"):
            # csrc/crop.hip per call, the workspace fill included, on AB_P particles (4096; 512 takes the 8-pixel
            # form's split of four): the bf16 crop of ViT-B/16 (224 x 224 frame, 64 x 64 box, S = 224, patch 16),
            # upright or with an angle row, and the colour cues (C = 32, B = 8: histograms, scores and Q)
            n = int(os.environ.get("AB_P", 4096))
            size = f"P={n}"
            frame = torch.randint(0, 256, (224, 224, 3), device=dev, dtype=torch.uint8, generator=g)
            ws = ops.rgba_workspace((224, 224), dev)
            u = torch.rand(4, n, device=dev, generator=g)
            state = torch.stack([u[0] * 224, u[1] * 224, 0.8 + 0.45 * u[2]]).contiguous()
            ang = ((u[3] * 2 - 1) * 3.14159).contiguous()
            ab = torch.tensor([1 / (255 * s) for s in (0.229, 0.224, 0.225)]
                              + [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]).numpy()
            tmpl = torch.rand(512, device=dev, generator=g)
            tmpl /= tmpl.sum()
            if case.startswith("crop"):
                bufs = {k: torch.empty(n * 196, 768, device=dev, dtype=torch.bfloat16) for k in ("product", "other")}
            else:
                bufs = {k: tuple([torch.empty(n, 512, device=dev, dtype=torch.int32) for _ in range(1 + (case != "color"))]
                                 + [torch.empty(n, device=dev) for _ in range(1 + (case != "color"))]
                                 + [torch.empty(n, device=dev, dtype=torch.int64)]) for k in ("product", "other")}

            def call(L, k):
                head = (pt(frame), 224, 224, pt(ws))
                if case == "crop":
                    return L.vpf_crop_patches_bf16(*head, pt(state), n, n, 64.0, 64.0, 224, 16, 768,
                                                   ab.ctypes.data_as(ctypes.c_void_p), pt(bufs[k]), st)
                if case == "crop_rot":
                    return L.vpf_crop_patches_rot_bf16(*head, pt(state), n, pt(ang), n, 64.0, 64.0, 224, 16, 768,
                                                       ab.ctypes.data_as(ctypes.c_void_p), pt(bufs[k]), st)
                if case == "color":
                    h, rho, q = bufs[k]
                    return L.vpf_color_weight(*head, 1, pt(state), n, None, n, 64.0, 64.0, 32, 8, pt(tmpl), 20.0, 40, 0,
                                              pt(h), pt(rho), pt(q), st)
                h, hs, rho, rho_s, q = bufs[k]
                return L.vpf_color_weight_surround(*head, 1, pt(state), n, None, n, 64.0, 64.0, 32, 8, pt(tmpl), 20.0,
                                                   10.0, 40, 0, pt(h), pt(hs), pt(rho), pt(rho_s), pt(q), st)
            flop = 0.0
        elif case == "quant":
            x = (torch.randn(M, 768, device=dev, generator=g) * 3).to(torch.bfloat16)
            bufs = {k: ops.mx8_empty(M, 768, dev) for k in ("product", "other")}

            def call(L, k):
                q, s = bufs[k]
                return L.vpf_quantize_mx8(pt(x), 768, M, 768, 1, pt(q), q.stride(0), pt(s), s.shape[1], st)
            flop = 0.0
        elif case.startswith("bf16_"):
            # the bf16 GEMMs with their product epilogues: qkv (LN fold), proj / fc2 (residual in place + statistics
            # planes), fc1 (LN fold + GELU); LN statistics planes of the A operand itself
            N, K, epi = {"bf16_qkv": (2304, 768, E.VPF_EPI_LN), "bf16_proj": (768, 768, E.VPF_EPI_BIAS_RESIDUAL),
                         "bf16_fc1": (3072, 768, E.VPF_EPI_LN_GELU),
                         "bf16_fc2": (768, 3072, E.VPF_EPI_BIAS_RESIDUAL)}[case]
            a = (torch.rand(M, K, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
            w = ((torch.rand(N, K, device=dev, generator=g) * 2 - 1) * 0.05).to(torch.bfloat16)
            bias = torch.rand(N, device=dev, generator=g) * 0.1
            colsum = w.float().sum(1).contiguous()
            # AB_PARTS=0: the encoder's form since round 5 ({mean, rstd} rows, combined by vpf_stats_combine before the GEMM)
            parts = int(os.environ.get("AB_PARTS", K // 64))
            if parts:
                af = a.float().view(M, parts, K // parts)
                planes = torch.stack([af.sum(2), (af * af).sum(2)], 2).transpose(0, 1).contiguous()   # [P][M][2]
            else:
                planes = torch.stack([torch.rand(M, device=dev, generator=g) * 0.2 - 0.1,
                                      torch.rand(M, device=dev, generator=g) + 0.5], 1).contiguous()   # [M][2]
            res0 = (torch.rand(M, N, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
            resid = epi == E.VPF_EPI_BIAS_RESIDUAL
            bufs = {}
            for k in ("product", "other"):
                out = res0.clone() if resid else torch.empty(M, N, device=dev, dtype=torch.bfloat16)
                bufs[k] = (out, torch.empty(N // 64, M, 2, device=dev) if resid else None)

            def call(L, k, reset=False):
                out, so = bufs[k]
                if resid and reset:
                    out.copy_(res0)
                return L.vpf_gemm_bf16(pt(a), K, pt(w), pt(bias), pt(out) if resid else None, None, 0,
                                       None if resid else pt(planes), None if resid else pt(colsum), pt(out), N, M, N, K,
                                       epi, 0 if resid else parts, 1e-6, pt(so) if resid else None, None, 0, None, 0,
                                       st)
            flop = 2.0 * M * N * K
        else:
            N, K = {"mx8_fc1": (3072, 768), "mx8_fc2": (768, 3072), "mx8_qkv": (2304, 768), "mx8_proj": (768, 768)}[case]
            a = (torch.rand(M, K, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
            w = ((torch.rand(N, K, device=dev, generator=g) * 2 - 1) * 0.05).to(torch.bfloat16)
            a8, as8 = ops.mx8_empty(M, K, dev)
            w8, ws8 = ops.mx8_empty(N, K, dev)
            V.quantize_mx8_(a, 1, a8, as8)
            V.quantize_mx8_(w, 1, w8, ws8)
            bias = torch.rand(N, device=dev, generator=g) * 0.1
            colsum = w.float().sum(1).contiguous()
            Pn = 0                                     # the product's LN form: one combined {mean, rstd} plane
            planes = torch.rand(M, 2, device=dev, generator=g) + 0.5
            res0 = (torch.rand(M, N, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
            bufs = {}
            for k in ("product", "other"):
                out = res0.clone() if case in ("mx8_fc2", "mx8_proj") else torch.empty(M, N, device=dev, dtype=torch.bfloat16)
                q8, s8 = ops.mx8_empty(M, N, dev)
                bufs[k] = (out, q8, s8, torch.empty((N + 63) // 64, M, 2, device=dev))
            epi = {"mx8_fc1": E.VPF_EPI_LN_GELU, "mx8_fc2": E.VPF_EPI_BIAS_RESIDUAL, "mx8_qkv": E.VPF_EPI_LN,
                   "mx8_proj": E.VPF_EPI_BIAS_RESIDUAL}[case]

            def call(L, k, reset=False):
                out, q8, s8, pl = bufs[k]
                fc1, fc2 = case == "mx8_fc1", case in ("mx8_fc2", "mx8_proj")
                if fc2 and reset:                      # the residual is read in place: same input for the bit check
                    out.copy_(res0)
                return L.vpf_gemm_mx8(pt(a8), a8.stride(0), pt(as8), as8.shape[1], pt(w8), pt(ws8), pt(bias),
                                      pt(out) if fc2 else None, None if fc2 else pt(planes),
                                      None if fc2 else pt(colsum), None if fc1 else pt(out), N, pt(q8) if fc1 or fc2 else None,
                                      q8.stride(0), pt(s8) if fc1 or fc2 else None, s8.shape[1], M, N, K, epi,
                                      0 if fc2 else Pn, 1e-6, pt(pl) if fc2 else None, st)
            flop = 2.0 * M * N * K
        for k, L in (("product", P), ("other", O)):
            assert (call(L, k, reset=True) if case.startswith(("mx8", "bf16")) else call(L, k)) == 0, (case, k)
        torch.cuda.synchronize()
        def snap(k):   # the outputs the call writes
            b = bufs[k]
            if case == "mx8_fc1":
                b = b[1:3]
            elif case == "mx8_qkv" or case in ("bf16_qkv", "bf16_fc1"):
                b = b[:1]
            return [t.clone() for t in (b if isinstance(b, (tuple, list)) else (b,)) if t is not None]
        same = all(torch.equal(x, y) for x, y in zip(snap("product"), snap("other")))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = {"product": [], "other": []}
        for r in range(rounds):
            for k, L in ((("product", P), ("other", O)) if r % 2 == 0 else (("other", O), ("product", P))):
                ev[0].record()
                for _ in range(3):
                    call(L, k)
                ev[1].record()
                torch.cuda.synchronize()
                times[k].append(ev[0].elapsed_time(ev[1]) / 3)
        for k in times:
            t = sorted(times[k])
            med = t[len(t) // 2]
            extra = f"  {flop / med / 1e9:.1f} TFLOP/s" if flop else ""
            print(f"{case:8s} {k:8s} {size}  median {med:.4f} ms (min {t[0]:.4f}, max {t[-1]:.4f}){extra}", flush=True)
        print(f"{case:8s} outputs bit-identical: {same}", flush=True)
        del bufs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
