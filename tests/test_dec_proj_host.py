"""CPU: the reference module of the decode-projection tests (tests/dec_proj_np.py) checked against itself —
the fragment-major pack / unpack helpers for every lean_cfg entry, the folded LayerNorm algebra against
LayerNorm + GEMM in fp64, and the 16-bit emulation of the fold inside the two bounds tests/test_gpu_dec_proj.py
asserts, on exactly its input recipe (the CPU-checked condition on those bounds)."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dec_proj_np as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lean_cfg_table_mirrors_the_header():
    src = open(os.path.join(ROOT, "whisper_context_biasing_amd", "csrc", "kernels.h")).read()
    body = src[src.index("inline bool lean_cfg"):]
    body = body[:body.index("default:")]
    got = {int(k): (int(a), int(b)) for k, a, b in re.findall(r"case (\d+): nw = (\d+); kpw = (\d+);", body)}
    assert got == R.LEAN_CFG
    assert all(nw * kpw * 32 == K for K, (nw, kpw) in R.LEAN_CFG.items())


@pytest.mark.parametrize("K", sorted(R.LEAN_CFG))
@pytest.mark.parametrize("rows", [16, 48])
def test_fragment_major_round_trip(K, rows):
    nw, kpw = R.LEAN_CFG[K]
    A = torch.arange(rows * K, dtype=torch.int64).reshape(rows, K)
    F = R.frag_pack(A, nw, kpw)
    assert F.shape == (rows // 16, nw, kpw, 64, 8)
    assert torch.equal(R.frag_unpack(F, rows, K), A)
    flat = F.reshape(-1)
    # the index formula of embed_kernel / dec_lean_kernel, element by element on a sample of (row, column)
    g = torch.Generator().manual_seed(K + rows)
    for r, k in zip(torch.randint(0, rows, (200,), generator=g).tolist(), torch.randint(0, K, (200,), generator=g).tolist()):
        assert flat[R.frag_index(r, k, nw, kpw)] == A[r, k]
    # frag_major's weight layout, read back lane by lane: dst[ct][wave][ks][lane][e] = W[16 ct + lane % 16][...]
    ct, wave, ks, lane, e = rows // 16 - 1, nw - 1, kpw - 1, 37, 5
    assert F[ct, wave, ks, lane, e] == A[16 * ct + lane % 16, wave * kpw * 32 + ks * 32 + 8 * (lane // 16) + e]


@pytest.mark.parametrize("K", sorted(R.LEAN_CFG))
def test_fragment_major_agrees_with_the_kernel_tests_helper(K):
    """_frag_major of test_gpu_kernels.py ([N / 16][K / 32][64][8]) is the same layout: (wave, k-step) is the
    32-deep k-step index in order, so the layouts coincide for every split."""
    from test_gpu_kernels import _frag_major
    nw, kpw = R.LEAN_CFG[K]
    W = torch.arange(32 * K, dtype=torch.int64).reshape(32, K)
    assert torch.equal(R.frag_pack(W, nw, kpw).reshape(32, K), _frag_major(W))


@pytest.mark.parametrize("K", [512, 768, 1280])
@pytest.mark.parametrize("mean_sigma,outliers", [(0, 0), (4, 1), (30, 0), (30, 1)])
def test_folded_algebra_equals_layernorm_gemm_in_fp64(K, mean_sigma, outliers):
    x = R.make_rows(K + mean_sigma, 37, K, mean_sigma, outliers)
    gam, bet, W, bias = R.make_weights(K, 128, K, torch.float32)
    mu, r = R.stats64(x)
    Wg = gam.double()[None, :] * W.double()
    u, c = Wg.sum(1), (bet.double()[None, :] * W.double()).sum(1) + bias.double()
    fold = r * (x.double() @ Wg.T - mu * u[None, :]) + c[None, :]
    ref = R.ref_true(x, gam, bet, W, bias)
    assert ((fold - ref).abs() / (ref.abs() + 1)).max().item() < 1e-12


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [512, 768, 1280])
@pytest.mark.parametrize("mean_sigma", [0, 4, 30])
@pytest.mark.parametrize("outliers", [0, 1])
@pytest.mark.parametrize("stats_of", ["x16", "f32"])
def test_emulated_fold_is_inside_both_bounds(dt, K, mean_sigma, outliers, stats_of):
    """The 16-bit emulation of r·(Σ x16·W' − μ·u) + c on the GPU test's recipe stays inside both bounds (the ratios
    are printed and tabulated in DESIGN.md §4a: up to 0.5 of the true bound; the same-input ratio is mostly the
    half ulp of the output rounding against ε·|ref|), so a correct kernel has room inside both."""
    M, N = 37, 128
    x = R.make_rows(K * 7 + M, M, K, mean_sigma, outliers)
    gam, bet, W, bias = R.make_weights(K + N, N, K, dt)
    rows = x if stats_of == "f32" else None
    out, x16, Wg, u, c = R.emulate_fold(x, gam, bet, W, bias, stat_rows=rows)
    srows = x if stats_of == "f32" else x16.float()
    same = R.ref_same_fold(srows, x16, Wg, u, c)
    true = R.ref_true(x, gam, bet, W, bias)
    r_same = R.ratio(out, same, R.bound_same(srows, x16.abs(), Wg.abs(), K, same, dt))
    r_true = R.ratio(out, true, R.bound_true(x, gam, W, true, dt))
    rel = ((out.double() - true).abs() / (true.abs() + 1)).max().item()
    o = R.ordinary_rows(M)   # (the all-zero row sits at half an output ulp of c: up to 1.0 of ε·|ref| by itself)
    o_same = R.ratio(out[o], same[o], R.bound_same(srows, x16.abs(), Wg.abs(), K, same, dt)[o])
    o_true = R.ratio(out[o], true[o], R.bound_true(x, gam, W, true, dt)[o])
    print(f"fold-emulation {str(dt)[6:]} K={K} mean={mean_sigma}s outl={outliers} stats={stats_of}: "
          f"same {o_same:.4f} true {o_true:.4f} (all rows {r_same:.3f} {r_true:.3f}) rel {rel:.4f}")
    assert torch.isfinite(out.float()).all()
    assert r_same < 1.0, r_same
    assert r_true < 1.0, r_true


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_special_rows_come_out_as_c(dt):
    """The all-zero row is exactly T(c_n) under the fold; the constant row is c_n up to r·(f32 sum-order error)."""
    K, N, M = 768, 128, 37
    x = R.make_rows(5, M, K, 4, 1)
    gam, bet, W, bias = R.make_weights(6, N, K, dt)
    out, x16, Wg, u, c = R.emulate_fold(x, gam, bet, W, bias)
    zr, on = R.special_rows(M)
    assert torch.equal(out[zr], c.float().to(dt))
    same = R.ref_same_fold(x16.float(), x16, Wg, u, c)
    b = R.bound_same(x16.float(), x16.abs(), Wg.abs(), K, same, dt)
    assert ((out[on].double() - c).abs() <= b[on] + R.EPS[dt] * c.abs()).all()
