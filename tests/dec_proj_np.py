"""fp64 references, input recipe and error bounds of the decode-step projection tests (tests/test_gpu_dec_proj.py,
tests/test_dec_proj_host.py). torch on the CPU only: the 16-bit roundings are torch's (round to nearest even, the
kernels' DT<T>::fromf).

Two references per LayerNorm-fused launch:
  same-input  fp64 of the algebra on the operands the kernel consumes — the 16-bit rows x16, the rounded W' = T(γ·W),
              u and c as prepared — with the exact (μ, r) of the rows the kernel takes its statistics from: x16 for
              the <= 64-row kernels (they sum the fragments they load), the f32 rows for the > 64-row tiles (rst_in is
              published from the f32 values). Bound: f32 accumulation 4·K·2^-24 · r·Σ_k |x16_k||W'_nk| + one output
              rounding ε·|ref| (ε = 2^-8 bf16, 2^-11 f16; an output below the format's smallest normal number is
              rounded on the fixed subnormal grid: ε·max(|ref|, 2^-14) for f16, `rounding`).
  true        fp64 LayerNorm of the f32 rows, W, bias, erf-GELU. Bound: ε · r·Σ_k |x_k||γ_k W_nk| + ε·|ref|.
Through GELU both bounds are scaled by its Lipschitz constant (max |GELU'| = 1.129 → 1.13) plus 1e-6 for the kernels'
erfc polynomial (Abramowitz-Stegun 7.1.26, |err| <= 1.5e-7)."""
import math

import torch

EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
GELU_LIP, GELU_ABS = 1.13, 1e-6
# smallest normal number of the format: below it the spacing stops shrinking, so one rounding costs up to
# ε·MIN_NORMAL (half the subnormal spacing), not ε·|ref|
MIN_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}


def rounding(ref, dt):
    """the most one round-to-nearest of ref to the format can move it: half a spacing, ε·max(|ref|, smallest normal)."""
    return EPS[dt] * ref.abs().clamp_min(MIN_NORMAL[dt])
# kernels.h lean_cfg: K -> (waves, 32-deep k-steps per wave)
LEAN_CFG = {64: (2, 1), 512: (4, 4), 768: (4, 6), 1024: (4, 8), 1280: (8, 5), 2048: (8, 8), 3072: (8, 12),
            4096: (16, 8), 5120: (16, 10)}


# ------------------------------------------------------------------------------------------------ fragment-major
def frag_pack(A, nw, kpw):
    """[R][K] (R % 16 == 0, K = nw·kpw·32) -> [R / 16][nw][kpw][64 lanes][8]: element (r, k) of row block r / 16 at wave
    k / (kpw·32), k-step (k % (kpw·32)) / 32, lane 16·((k % 32) / 8) + r % 16, slot k % 8 — the layout of frag_major
    (weights, r = output column) and of embed_kernel / dec_lean_kernel (activations, r = row)."""
    R, K = A.shape
    assert R % 16 == 0 and K == nw * kpw * 32, (R, K, nw, kpw)
    return A.reshape(R // 16, 16, nw, kpw, 4, 8).permute(0, 2, 3, 4, 1, 5).reshape(R // 16, nw, kpw, 64, 8).contiguous()


def frag_unpack(F, R, K):
    nb, nw, kpw = F.shape[0], F.shape[1], F.shape[2]
    assert nb * 16 == R and nw * kpw * 32 == K
    return F.reshape(nb, nw, kpw, 4, 16, 8).permute(0, 4, 1, 2, 3, 5).reshape(R, K).contiguous()


def frag_index(r, k, nw, kpw):
    """flat element offset of (r, k): embed_kernel's index formula restated."""
    kw = kpw * 32
    return ((((r >> 4) * nw + k // kw) * kpw + ((k % kw) >> 5)) * 64 + ((k & 31) >> 3) * 16 + (r & 15)) * 8 + (k & 7)


# ------------------------------------------------------------------------------------------------ inputs
def make_rows(seed, M, K, mean_sigma, outliers):
    """f32 rows: randn + a per-row mean of mean_sigma·σ (σ of the row with its outliers), two outlier columns (x50,
    x30) when asked; M >= 5: row 1 all zeros, row 2 the constant 1.0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    if outliers:
        x[:, 7] *= 50
        x[:, K - 3] *= 30
    x = x + mean_sigma * x.std(1, keepdim=True)
    if M >= 5:
        x[1] = 0.0
        x[2] = 1.0
    return x.float()


def special_rows(M):
    return (1, 2) if M >= 5 else ()


def ordinary_rows(M):
    return [i for i in range(M) if i not in special_rows(M)]


def make_weights(seed, N, K, dt):
    g = torch.Generator().manual_seed(seed)
    gam = (1 + 0.3 * torch.randn(K, generator=g)).float()
    bet = (0.2 * torch.randn(K, generator=g)).float()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dt)
    bias = torch.randn(N, generator=g).float()
    return gam, bet, W, bias


# ------------------------------------------------------------------------------------------------ references
def stats64(rows):
    """exact (μ, r = 1 / sqrt(var + 1e-5)) of the rows, fp64 [M][1]."""
    xd = rows.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    return mu, 1.0 / torch.sqrt(var + 1e-5)


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def ln64(x, gam, bet):
    mu, r = stats64(x)
    return (x.double() - mu) * r * gam.double() + bet.double()


def ref_true(x, gam, bet, W, bias, gelu=False):
    v = ln64(x, gam, bet) @ W.double().T + bias.double()
    return gelu64(v) if gelu else v


def fold_operands(gam, bet, W, bias):
    """W' = T(γ·W) (f32 product, one rounding: scale_cols), u = Σ_k W'[n][k], c = Σ_k β_k W[n][k] + b[n], fp64."""
    Wg = (gam[None, :] * W.float()).to(W.dtype)
    return Wg, Wg.double().sum(1), (bet.double()[None, :] * W.double()).sum(1) + bias.double()


def ref_same_fold(stat_rows, x16, Wg, u, c, gelu=False):
    mu, r = stats64(stat_rows)
    v = r * (x16.double() @ Wg.double().T - mu * u.double()[None, :]) + c.double()[None, :]
    return gelu64(v) if gelu else v


def ref_same_unfold(ln_rows, gam, bet, W, bias, gelu=False):
    """A = T(LN(rows)) in fp64, then the product on the 16-bit A (the unfolded paths)."""
    A = ln64(ln_rows, gam, bet).to(W.dtype)
    v = A.double() @ W.double().T + bias.double()
    return (gelu64(v) if gelu else v), A


def bound_same(stat_rows, a_abs, W_abs, K, ref, dt, gelu=False, r_scale=True):
    """4·K·2^-24 · r·Σ|a||w| + ε|ref| (r_scale False: a is already normalised — the unfolded paths, RESID)."""
    r = stats64(stat_rows)[1] if r_scale else 1.0
    b = 4.0 * K * 2.0 ** -24 * r * (a_abs.double() @ W_abs.double().T)
    if gelu:
        b = GELU_LIP * b + GELU_ABS
    return b + rounding(ref, dt)


def bound_true(x, gam, W, ref, dt, gelu=False):
    _, r = stats64(x)
    b = EPS[dt] * r * (x.double().abs() @ (gam.double().abs()[None, :] * W.double().abs()).T)
    if gelu:
        b = GELU_LIP * b + GELU_ABS
    return b + rounding(ref, dt)


def ratio(out, ref, bound):
    """max over the elements of |out − ref| / bound (a bound of 0 with an exact output counts 0)."""
    err = (out.double() - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max())


def emulate_fold(x, gam, bet, W, bias, stat_rows=None, gelu=False):
    """the folded kernels' arithmetic on the CPU: f32 statistics Σx²/K − μ², f32 accumulation, one output rounding."""
    dt = W.dtype
    x16 = x.to(dt)
    Wg, u, c = fold_operands(gam, bet, W, bias)
    s = (x16.float() if stat_rows is None else stat_rows)
    K = x.shape[1]
    mean = s.sum(1, keepdim=True) / K
    rstd = torch.rsqrt(torch.clamp((s * s).sum(1, keepdim=True) / K - mean * mean, min=0) + 1e-5)
    acc = x16.float() @ Wg.float().T
    v = rstd * (acc - mean * u.float()[None, :]) + c.float()[None, :]
    if gelu:
        v = torch.nn.functional.gelu(v)
    return v.to(dt), x16, Wg, u, c


def partial_stats(x, w):
    """[M][K / w][2] fp64 (Σx, Σx²) per w columns."""
    M, K = x.shape
    xd = x.double().reshape(M, K // w, w)
    return torch.stack([xd.sum(2), (xd * xd).sum(2)], dim=2)
