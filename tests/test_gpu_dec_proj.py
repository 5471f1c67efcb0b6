"""GPU: kernel-level parity of the decode-step projections (wcb_op_dec_proj) and the step embedding (wcb_op_embed).

One launch of the decoder's layer loop at a time, on caller operands, against the fp64 references of
tests/dec_proj_np.py. Every LayerNorm-fused launch is held to two bounds (see that module): the same-input reference
pins the kernel's arithmetic, the true reference bounds the formulation (16-bit rows that are not centred before the
product). Inputs: rows of mean 0 / 4σ / 30σ, outlier columns in half the cases, an all-zero row and a constant row;
every row-indexed operand is padded to 64 rows with NaN, every output with a sentinel: no NaN may reach a valid
row and no sentinel row or foreign cache slot may change. Every case runs twice, bit-identical, and asserts through
`taken` which launcher ran. Each test prints `dec-proj-ratio ...` lines: the largest error / bound per path (the
figures of DESIGN.md §4a).

Special rows. Under the fold the all-zero row must be exactly T(c_n); the constant row, and both rows on the unfolded
paths (A = T(β)), must be within ε·|c_n| + the same-input accumulation bound (+ ε·Σ|β_k||W_nk| for the rounding of
A = T(β) where the LayerNorm is not folded, + the f32 preparation of c_n itself, 2^-22·(Σ|β_k W_nk| + |b_n|)) of
c_n = Σ β_k W_nk + b_n. The true-reference bound, which has no β
term, is asserted on the ordinary rows.

QKV with several positions per row (kv_rps = 3, the general decode GEMM and the tiles) needs M % 3 == 0 and
*pos + 3 <= T: those cases use the multiples of 3 next to the listed row counts and pos in {0, 3, T − 3}.

Combinations that are not defined (wcb_op_dec_proj returns WCB_ERR_UNSUPPORTED; test_undefined_combinations_are_refused
asserts it, nothing is skipped): see UNDEFINED below.
"""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dec_proj_np as R  # noqa: E402
from whisper_context_biasing_amd import _lib as L  # noqa: E402

DT = {"bf16": (torch.bfloat16, L.WCB_BF16), "f16": (torch.float16, L.WCB_F16), "f32": (torch.float32, L.WCB_F32)}
SENT = -777.0
MS = [1, 5, 16, 17, 33, 64]
KDT = [(512, "bf16"), (768, "bf16"), (1024, "bf16"), (1280, "bf16"), (768, "f16"), (1280, "f16")]
LN_KINDS = {"plain": L.PROJ_LN_PLAIN, "gelu": L.PROJ_LN_GELU, "qkv": L.PROJ_QKV}
PATHS64 = {"dec": L.PATH_DEC, "lean": L.PATH_LEAN, "fold": L.PATH_LEAN_FOLD, "foldfm": L.PATH_LEAN_FOLD_FM}
PATHS_T = {"lnring": L.PATH_LN_RING, "ringfold": L.PATH_RING_FOLD, "wide": L.PATH_WIDE}
WANT = {"dec": L.TAKEN_DEC_MF, "lean": L.TAKEN_LEAN, "fold": L.TAKEN_LEAN, "foldfm": L.TAKEN_LEAN,
        "lnring": L.TAKEN_RING_DEC, "ringfold": L.TAKEN_RING_DEC, "wide": L.TAKEN_WIDE}
# (kind, path) pairs the entry point refuses whatever the shape: 9 of the 6 x 7 pairs
UNDEFINED = [
    ("qkv", "wide"),                                   # QKV keeps the ring tiles (decode_rows: !kv_out)
    ("kq", "lnring"), ("kq", "ringfold"), ("kq", "wide"),   # grouped products stay on the decode kernels
    ("xqk", "dec"), ("xqk", "lean"),                   # the fused cross query exists for the folded lean form only
    ("xqk", "lnring"), ("xqk", "ringfold"), ("xqk", "wide"),
]


def _s():
    return torch.cuda.current_stream().cuda_stream


def sync(rc=0):
    """after a HIP error nothing more is launched: the session ends there."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # an asynchronous GPU fault surfaces here
        pytest.exit(f"GPU fault: {e}", returncode=3)
    if rc == -3:
        pytest.exit(f"HIP error: {L.load().wcb_last_error(None)}", returncode=3)


def pad(t, rows, fill):
    out = torch.full((rows,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    out[:t.shape[0]] = t
    return out.cuda()


def up(n, m):
    return (n + m - 1) // m * m


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def proj(kind, path, dt, M, N, K, expect_rc=0, **kw):
    lib = L.load()
    p = L.WcbDecProj(kind=kind, path=path, dtype=DT[dt][1], M=M, N=N, K=K)
    for k, v in kw.items():
        setattr(p, k, v.data_ptr() if torch.is_tensor(v) else v)
    tk = C.c_int32(-1)
    p.taken = C.pointer(tk)
    rc = lib.wcb_op_dec_proj(C.byref(p), _s())
    sync(rc)
    assert rc == expect_rc, (rc, lib.wcb_last_error(None))
    return tk.value


def report(tag, **ratios):
    print("dec-proj-ratio " + tag + " " + " ".join(f"{k}={v:.4f}" for k, v in ratios.items()))


def twice(fn):
    a, b = fn(), fn()
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(bits(a[k]), bits(b[k])), "not bit-identical: " + k
        else:
            assert a[k] == b[k], k
    return a


# ------------------------------------------------------------------------------------------------ LN-fused launches
def ln_launch(kind, path, dt, M, N, K, x, gam, bet, W, bias, *, pos=0, T=8, rps=1, ring_kt=1, a_fm=None, x16=None,
              rst=None, out_fm=0):
    """One LN-fused launch on padded operands -> dict of outputs (CPU) and the folded operands."""
    tdt = DT[dt][0]
    Mp = up(M, 64)
    x16 = x.to(tdt) if x16 is None else x16
    kw = dict(ln_w=gam.cuda(), ln_b=bet.cuda(), W=W.cuda(), bias=bias.cuda(), x=pad(x, Mp, float("nan")),
              a16=pad(x16, Mp, float("nan")), ring_kt=ring_kt)
    pname = [k for k, v in {**PATHS64, **PATHS_T}.items() if v == path][0]
    if pname == "foldfm":
        nw, kpw = R.LEAN_CFG[K]
        kw["a_fm"] = a_fm if a_fm is not None else R.frag_pack(pad(x16, Mp, float("nan")).cpu(), nw, kpw).cuda()
    if pname in ("ringfold", "wide"):
        kw["rst_in"] = rst if rst is not None else pad(R.partial_stats(x, 32).float(), Mp, float("nan"))
    if pname in ("fold", "foldfm", "ringfold", "wide"):
        kw.update(u_out=torch.empty(N, device="cuda"), c_out=torch.empty(N, device="cuda"),
                  wg_out=torch.empty(N, K, dtype=tdt, device="cuda"))
    qkv = kind == L.PROJ_QKV
    n_out = K if qkv else N
    out = torch.full((Mp, n_out), SENT, dtype=tdt, device="cuda")
    if out_fm:
        kw["out_fm"] = 1
    kw["out"] = out
    if qkv:
        H, B = K // 64, M // rps + 1
        kv = torch.full((2, B, H, T, 64), SENT, dtype=tdt, device="cuda")
        kw.update(kv=kv, pos=torch.tensor([pos], dtype=torch.int32, device="cuda"), kv_B=B, kv_T=T, kv_rps=rps, n_split=K)
    taken = proj(kind, path, dt, M, N, K, **kw)
    res = dict(out=out.cpu(), taken=taken)
    if qkv:
        res["kv"] = kv.cpu()
    for k in ("u_out", "c_out", "wg_out"):
        if k in kw:
            res[k] = kw[k].cpu()
    return res


def ln_check(tag, kind, pname, dt, M, N, K, x, gam, bet, W, bias, res, *, pos=0, T=8, rps=1, stat_rows=None, x16=None,
             special=True):
    """res against the two references; returns (same ratio, true ratio) over the ordinary rows. special: x is
    make_rows' (rows 1 and 2 all-zero and constant); False for rows another launch wrote (the chains): every row is
    ordinary."""
    tdt = DT[dt][0]
    gelu = kind == L.PROJ_LN_GELU
    qkv = kind == L.PROJ_QKV
    x16 = x.to(tdt) if x16 is None else x16
    folded = pname in ("fold", "foldfm", "ringfold", "wide")
    # the rows the launcher takes its statistics from (module docstring of dec_proj_np)
    srows = stat_rows if stat_rows is not None else (x if pname in ("lnring", "ringfold", "wide") else x16.float())
    true = R.ref_true(x, gam, bet, W, bias, gelu)
    b_true = R.bound_true(x, gam, W, true, tdt, gelu)
    if folded:
        Wg, u, c = res["wg_out"], res["u_out"], res["c_out"]
        Wg_ref, u_ref, c_ref = R.fold_operands(gam, bet, W, bias)
        bad = (bits(Wg) != bits(Wg_ref)).nonzero()
        if len(bad):
            n, k = bad[0].tolist()
            print(f"dec-proj-wg {tag}: {len(bad)} of {Wg.numel()} elements differ from T(γ·W), first ({n}, {k}): W {W[n, k].item()!r} "
                  f"γ {gam[k].item()!r} got {Wg[n, k].item()!r} want {Wg_ref[n, k].item()!r}")
        # T(γ·W): the f16 build rounds the exact product once (a fused multiply-convert) where the f32 product
        # rounded again lands on the other side of a tie (measured: 17 of 147,456 elements at K = 768) — either
        # way no further from the exact product than the twice-rounded reference
        exact = gam.double()[None] * W.double()
        assert ((Wg.double() - exact).abs() <= (Wg_ref.double() - exact).abs() * (1 + 1e-9)).all(), "W' is not T(γ·W)"
        u_ref = Wg.double().sum(1)   # of the W' the launch multiplies (f32 wave sums: 2^-22 relative to Σ|W'|)
        assert ((u.double() - u_ref).abs() <= 2.0 ** -22 * Wg.double().abs().sum(1) + 1e-30).all()
        assert ((c.double() - c_ref).abs() <= 2.0 ** -22 * ((bet.double().abs()[None] * W.double().abs()).sum(1) + bias.abs())).all()
        same = R.ref_same_fold(srows, x16, Wg, u, c, gelu)
        b_same = R.bound_same(srows, x16.abs(), Wg.abs(), K, same, tdt, gelu)
        a_round = torch.zeros_like(same)
    else:
        same, A = R.ref_same_unfold(srows, gam, bet, W, bias, gelu)
        b_same = R.bound_same(None, A.abs(), W.abs(), K, same, tdt, gelu, r_scale=False)
        a_round = R.EPS[tdt] * (bet.double().abs()[None] * W.double().abs()).sum(1)[None].expand_as(same)
    # assemble the launch's [M][N] result: q rows + the appended cache slots
    out = res["out"]
    assert torch.equal(out[M:], torch.full_like(out[M:], SENT)), "a padded output row was written"
    got = out[:M].double()
    if qkv:
        kv = res["kv"]
        H, B = K // 64, kv.shape[1]
        mark = torch.zeros(kv.shape, dtype=torch.bool)
        cols = []
        for m in range(M):
            cols.append(kv[:, m // rps, :, pos + m % rps, :].reshape(2 * K))
            mark[:, m // rps, :, pos + m % rps, :] = True
        assert torch.equal(kv[~mark], torch.full_like(kv[~mark], SENT)), "a cache slot other than the appended ones changed"
        got = torch.cat([got, torch.stack(cols).double()], dim=1)
    assert torch.isfinite(got).all(), "NaN / inf in a valid row"
    o = R.ordinary_rows(M) if special else list(range(M))
    if R.ratio(got, same, b_same) > 1.0:   # (a bound is met with equality by a tie: <=)
        i = int(((got - same).abs() / b_same.clamp_min(1e-300)).argmax())
        m, n = i // got.shape[1], i % got.shape[1]
        raise AssertionError((tag, "same-input bound", R.ratio(got, same, b_same), "row", m, "column", n, "out", got[m, n].item(),
                              "ref", same[m, n].item(), "bound", b_same[m, n].item()))
    r_same, r_true = R.ratio(got[o], same[o], b_same[o]), R.ratio(got[o], true[o], b_true[o])
    assert r_true < 1.0, (tag, "true bound", r_true)
    if special and R.special_rows(M) and not gelu:
        zr, on = R.special_rows(M)
        c64 = (bet.double()[None] * W.double()).sum(1) + bias.double()
        if folded:
            assert torch.equal(bits(got[zr].to(tdt)), bits(res["c_out"].to(tdt))), "the all-zero row is not T(c)"
        # c_n itself is prepared in f32 (ln_fold's wave sums: 2^-22 relative to Σ|β_k W_nk| + |b_n|, asserted above);
        # where β·W cancels the bias that is all a tiny c_n has
        c_prep = 2.0 ** -22 * ((bet.double().abs()[None] * W.double().abs()).sum(1) + bias.double().abs())
        for row in (zr, on):
            acc = b_same[row] - R.rounding(same[row], tdt)
            assert ((got[row] - c64).abs() <= R.rounding(c64, tdt) + acc + a_round[row] + c_prep).all(), (tag, "special row", row)
    return r_same, r_true


def recipe(i):
    """(row mean in σ, outliers) of the i-th case: means cycle 0 / 4 / 30, outliers in every other one."""
    return (0, 4, 30)[i % 3], i % 2


@pytest.mark.parametrize("K,dt", KDT)
@pytest.mark.parametrize("pname", list(PATHS64))
@pytest.mark.parametrize("kname", list(LN_KINDS))
def test_ln_fused_projection_up_to_64_rows(kname, pname, K, dt):
    kind, path, tdt = LN_KINDS[kname], PATHS64[pname], DT[dt][0]
    N = 3 * K if kname == "qkv" else 192
    gam, bet, W, bias = R.make_weights(K + N, N, K, tdt)
    worst = [0.0, 0.0]
    cases = [(M, 1) for M in MS]
    if kname == "qkv" and pname == "dec":
        cases = [(3, 3), (15, 3), (18, 3), (33, 3), (63, 3), (1, 1), (17, 1), (64, 1)]
    for i, (M, rps) in enumerate(cases):
        ms, outl = recipe(i + K // 256)
        T = 8
        pos = (0, 3, T - rps)[i % 3]
        x = R.make_rows(K * 31 + M, M, K, ms, outl)
        res = twice(lambda: ln_launch(kind, path, dt, M, N, K, x, gam, bet, W, bias, pos=pos, T=T, rps=rps))
        assert res["taken"] & 255 == WANT[pname], (res["taken"], pname)
        rs, rt = ln_check(f"{kname}/{pname}/{dt}/K{K}/M{M}", kind, pname, dt, M, N, K, x, gam, bet, W, bias, res, pos=pos, T=T, rps=rps)
        worst = [max(worst[0], rs), max(worst[1], rt)]
    report(f"{kname} {pname} {dt} K={K}", same=worst[0], true=worst[1])


@pytest.mark.parametrize("K,dt", KDT)
@pytest.mark.parametrize("pname", list(PATHS64))
@pytest.mark.parametrize("kname", ["plain", "gelu"])
def test_ln_fused_projection_32_row_workgroups(kname, pname, K, dt):
    """N = 2048, M = 33: the lean LN-fused launches take 32-row workgroups (two row blocks per workgroup, the second
    workgroup with one valid row)."""
    kind, path, tdt = LN_KINDS[kname], PATHS64[pname], DT[dt][0]
    M, N = 33, 2048
    gam, bet, W, bias = R.make_weights(K + N, N, K, tdt)
    x = R.make_rows(K + 33, M, K, 30 if K % 512 else 4, 1)
    res = twice(lambda: ln_launch(kind, path, dt, M, N, K, x, gam, bet, W, bias))
    assert res["taken"] & 255 == WANT[pname]
    rs, rt = ln_check(f"{kname}/{pname}/{dt}/K{K}/mf2", kind, pname, dt, M, N, K, x, gam, bet, W, bias, res)
    report(f"{kname} {pname} {dt} K={K} N=2048", same=rs, true=rt)


# one shape per ring-tile branch of gemm_t (tile code 1: 64x64, 2: 64x32, 3: 32x32), ring_kt 1 and 2, and the wide tiles
TILE_SHAPES = [("qkv", 320, 3072, 1024, 1), ("qkv", 320, 2304, 768, 2), ("plain", 320, 3072, 768, 1), ("gelu", 320, 1536, 768, 2), ("plain", 70, 768, 768, 3),
               ("gelu", 96, 1280, 1280, 3), ("qkv", 72, 1536, 512, 3)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("ring_kt", [1, 2])
@pytest.mark.parametrize("pname", ["lnring", "ringfold"])
@pytest.mark.parametrize("kname,M,N,K,tile", TILE_SHAPES)
def test_ln_fused_projection_ring_tiles(kname, M, N, K, tile, pname, ring_kt, dt):
    kind, path, tdt = LN_KINDS[kname], PATHS_T[pname], DT[dt][0]
    gam, bet, W, bias = R.make_weights(K + N, N, K, tdt)
    ms, outl = recipe(M + ring_kt)
    x = R.make_rows(K + M, M, K, ms, outl)
    rps = 3 if kname == "qkv" and M % 3 == 0 else 1
    pos = 5 if rps == 3 else 7
    res = twice(lambda: ln_launch(kind, path, dt, M, N, K, x, gam, bet, W, bias, pos=pos, rps=rps, ring_kt=ring_kt))
    assert res["taken"] == L.TAKEN_RING_DEC + 256 * tile, res["taken"]
    rs, rt = ln_check(f"{kname}/{pname}/{dt}/M{M}N{N}K{K}", kind, pname, dt, M, N, K, x, gam, bet, W, bias, res, pos=pos, rps=rps)
    report(f"{kname} {pname} kt{ring_kt} {dt} M={M} N={N} K={K}", same=rs, true=rt)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("K", [768, 1280])
@pytest.mark.parametrize("M", [70, 80, 96])
@pytest.mark.parametrize("kname", ["plain", "gelu"])
def test_ln_fused_projection_wide_tiles(kname, M, K, dt):
    """wide tile 12 (xq) and 22 (fc1) with the folded LayerNorm and fragment-major W'."""
    kind, tdt = LN_KINDS[kname], DT[dt][0]
    N = K if kname == "plain" else 2048
    gam, bet, W, bias = R.make_weights(K + N, N, K, tdt)
    ms, outl = recipe(M // 10 + K // 256)
    x = R.make_rows(K + M, M, K, ms, outl)
    res = twice(lambda: ln_launch(kind, L.PATH_WIDE, dt, M, N, K, x, gam, bet, W, bias))
    assert res["taken"] == L.TAKEN_WIDE
    rs, rt = ln_check(f"{kname}/wide/{dt}/M{M}K{K}", kind, "wide", dt, M, N, K, x, gam, bet, W, bias, res)
    report(f"{kname} wide {dt} M={M} K={K}", same=rs, true=rt)


# ------------------------------------------------------------------------------------------------ residual writers
def resid_launch(path, dt, M, N, K, A, W, bias, x0, *, a_fm=None, want_fm=False, st16=False, rst32=False, ring_kt=1):
    tdt = DT[dt][0]
    Mp = up(M, 64)
    x = pad(x0, Mp, SENT)
    out16 = torch.full((Mp, N), SENT, dtype=tdt, device="cuda")
    kw = dict(W=W.cuda(), bias=bias.cuda(), x=x, out16=out16, ring_kt=ring_kt)
    if a_fm is not None:
        kw["a_fm"] = a_fm
    else:
        kw["a16"] = pad(A, Mp, float("nan"))
    if want_fm:
        kw["out16_fm"] = torch.full((Mp * N,), SENT, dtype=tdt, device="cuda")
    if st16:
        kw["st_out"] = torch.full((Mp, N // 16, 2), SENT, device="cuda")
    if rst32:
        kw["rst_out"] = torch.full((Mp, N // 32, 2), SENT, device="cuda")
    taken = proj(L.PROJ_RESID, path, dt, M, N, K, **kw)
    res = dict(x=x.cpu(), out16=out16.cpu(), taken=taken)
    for k in ("out16_fm", "st_out", "rst_out"):
        if k in kw:
            res[k] = kw[k].cpu()
    return res


def stats_check(st, xo, w, M):
    """[M][N / w][2] partials of the written f32 rows against fp64 sums: 32·2^-24 relative to Σ|x| and Σx²."""
    ref = R.partial_stats(xo, w)
    mag = torch.stack([xo.double().abs().reshape(M, -1, w).sum(2), ref[:, :, 1]], dim=2)
    assert ((st[:M].double() - ref).abs() <= 32 * 2.0 ** -24 * mag + 1e-30).all(), "row statistics partials"
    assert torch.equal(st[M:], torch.full_like(st[M:], SENT)), "a padded statistics row was written"


def resid_check(tag, dt, M, N, K, A, W, bias, x0, res):
    tdt = DT[dt][0]
    ref = x0.double() + A.double() @ W.double().T + bias.double()
    bound = 4.0 * K * 2.0 ** -24 * (A.double().abs() @ W.double().abs().T + x0.double().abs() + bias.double().abs())
    xo = res["x"]
    assert torch.equal(xo[M:], torch.full_like(xo[M:], SENT)) and torch.equal(res["out16"][M:], torch.full_like(res["out16"][M:], SENT))
    assert torch.isfinite(xo[:M]).all()
    r = R.ratio(xo[:M], ref, bound)
    assert r < 1.0, (tag, r)
    assert torch.equal(bits(res["out16"][:M]), bits(xo[:M].to(tdt))), "out16 is not T(x)"
    if "out16_fm" in res:
        nw, kpw = R.LEAN_CFG[N]
        Mp = xo.shape[0]
        want = R.frag_pack(torch.cat([xo[:M].to(tdt), torch.full((Mp - M, N), SENT, dtype=tdt)]), nw, kpw).reshape(-1)
        assert torch.equal(bits(res["out16_fm"]), bits(want)), "fragment-major copy"
    if "st_out" in res:
        stats_check(res["st_out"], xo[:M], 16, M)
    if "rst_out" in res:
        stats_check(res["rst_out"], xo[:M], 32, M)
    return r


def resid_inputs(seed, M, N, K, tdt, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(M, K, generator=g) * scale).to(tdt)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(tdt)
    bias = torch.randn(N, generator=g).float()
    x0 = R.make_rows(seed, M, N, 4, 1)
    return A, W, bias, x0


@pytest.mark.parametrize("K,dt", KDT + [(2048, "bf16"), (3072, "bf16"), (4096, "bf16"), (5120, "bf16")])
@pytest.mark.parametrize("pname", ["dec", "lean", "fold", "foldfm"])
def test_residual_writer_up_to_64_rows(pname, K, dt):
    """out / xo / fc2: x += A·Wᵀ + b in place, out16 = T(x) exactly; foldfm: A fragment-major in, the 16-bit rows
    fragment-major out as well; dec: the 16-column statistics of the older consumers; fold: the lean launch (a
    residual writer has no LayerNorm to fold)."""
    tdt = DT[dt][0]
    N = 512 if pname == "foldfm" else 192
    worst = 0.0
    for M in MS:
        A, W, bias, x0 = resid_inputs(K + M, M, N, K, tdt)
        a_fm = None
        if pname == "foldfm":
            nw, kpw = R.LEAN_CFG[K]
            a_fm = R.frag_pack(pad(A, up(M, 64), float("nan")).cpu(), nw, kpw).cuda()
        res = twice(lambda: resid_launch(PATHS64[pname], dt, M, N, K, A, W, bias, x0, a_fm=a_fm, want_fm=pname == "foldfm",
                                         st16=pname == "dec"))
        assert res["taken"] & 255 == WANT[pname]
        worst = max(worst, resid_check(f"resid/{pname}/{dt}/K{K}/M{M}", dt, M, N, K, A, W, bias, x0, res))
    report(f"resid {pname} {dt} K={K}", acc=worst)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("ring_kt", [1, 2])
@pytest.mark.parametrize("pname,M,N,K,tile", [("ringfold", 320, 768, 3072, 3), ("ringfold", 70, 768, 768, 3), ("lnring", 320, 1536, 768, 2),
                                              ("ringfold", 320, 3072, 768, 1), ("wide", 70, 768, 768, 0), ("wide", 80, 1280, 1280, 0),
                                              ("wide", 96, 768, 768, 0)])
def test_residual_writer_tiles(pname, M, N, K, tile, ring_kt, dt):
    tdt = DT[dt][0]
    A, W, bias, x0 = resid_inputs(K + M + N, M, N, K, tdt)
    res = twice(lambda: resid_launch(PATHS_T[pname], dt, M, N, K, A, W, bias, x0, rst32=pname != "lnring", ring_kt=ring_kt))
    assert res["taken"] == (L.TAKEN_WIDE if pname == "wide" else L.TAKEN_RING_DEC + 256 * tile), res["taken"]
    report(f"resid {pname} kt{ring_kt} {dt} M={M} N={N} K={K}", acc=resid_check("resid/tiles", dt, M, N, K, A, W, bias, x0, res))


# ------------------------------------------------------------------------------------------------ cross query
def kq_ref(q16, Wk, H, d):
    """q'_h[c] = Σ_i W_k[h·64 + i][c] · q[h·64 + i], fp64 -> [M][H·d], and Σ|·||·| for the bound."""
    q = q16.double().reshape(-1, H, 64)
    w = Wk.double().reshape(H, 64, d)
    return torch.einsum("mhi,hic->mhc", q, w).reshape(-1, H * d), torch.einsum("mhi,hic->mhc", q.abs(), w.abs()).reshape(-1, H * d)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("d", [512, 768, 1280])
@pytest.mark.parametrize("pname", ["dec", "lean", "fold", "foldfm"])
def test_grouped_cross_query(pname, d, dt):
    tdt, H = DT[dt][0], d // 64
    g = torch.Generator().manual_seed(d)
    Wk = (torch.randn(d, d, generator=g) / d ** 0.5).to(tdt)
    worst = 0.0
    for M in MS + ([70] if pname == "dec" else []):
        q = torch.randn(M, d, generator=g).to(tdt)
        Mp = up(M, 64)

        def run():
            out = torch.full((Mp, H * d), SENT, dtype=tdt, device="cuda")
            tk = proj(L.PROJ_KQ, PATHS64[pname], dt, M, d, d, Wk=Wk.cuda(), a16=pad(q, Mp, float("nan")), out=out)
            return dict(out=out.cpu(), taken=tk)
        res = twice(run)
        assert res["taken"] == WANT[pname]
        ref, mag = kq_ref(q, Wk, H, d)
        out = res["out"]
        assert torch.equal(out[M:], torch.full_like(out[M:], SENT)) and torch.isfinite(out[:M].float()).all()
        worst = max(worst, R.ratio(out[:M], ref, 4 * 64 * 2.0 ** -24 * mag + R.rounding(ref, tdt)))
    assert worst < 1.0, worst
    report(f"kq {pname} {dt} d={d}", acc=worst)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("nch", [2, 8])
@pytest.mark.parametrize("d", [512, 768, 1280])
@pytest.mark.parametrize("pname", ["fold", "foldfm"])
def test_fused_cross_query(pname, d, nch, dt):
    """XQK against KQ(LN_PLAIN(x)) built from the fp64 same-input reference with q rounded once to 16 bits. Bound: the
    grouped product's accumulation + output rounding, plus the q rows' own same-input bound carried through W_k
    (Σ_i |W_k[h·64 + i][c]| · bound_q[h·64 + i]) and one 16-bit ulp of q where that bound lets the rounding flip."""
    tdt, H = DT[dt][0], d // 64
    gam, bet, W, bias = R.make_weights(d * 3, d, d, tdt)
    g = torch.Generator().manual_seed(d + nch)
    Wk = (torch.randn(d, d, generator=g) / d ** 0.5).to(tdt)
    worst = 0.0
    for i, M in enumerate(MS):
        ms, outl = recipe(i + nch)
        x = R.make_rows(d + M + nch, M, d, ms, outl)
        x16, Mp = x.to(tdt), up(M, 64)
        nw, kpw = R.LEAN_CFG[d]

        def run():
            out = torch.full((Mp, H * d), SENT, dtype=tdt, device="cuda")
            kw = dict(ln_w=gam.cuda(), ln_b=bet.cuda(), W=W.cuda(), bias=bias.cuda(), Wk=Wk.cuda(), x=pad(x, Mp, float("nan")),
                      a16=pad(x16, Mp, float("nan")), out=out, xqk_nch=nch, u_out=torch.empty(d, device="cuda"),
                      c_out=torch.empty(d, device="cuda"), wg_out=torch.empty(d, d, dtype=tdt, device="cuda"))
            if pname == "foldfm":
                kw["a_fm"] = R.frag_pack(pad(x16, Mp, float("nan")).cpu(), nw, kpw).cuda()
            tk = proj(L.PROJ_XQK, PATHS64[pname], dt, M, d, d, **kw)
            return dict(out=out.cpu(), taken=tk, u=kw["u_out"].cpu(), c=kw["c_out"].cpu(), wg=kw["wg_out"].cpu())
        res = twice(run)
        assert res["taken"] == L.TAKEN_XQK
        q64 = R.ref_same_fold(x16.float(), x16, res["wg"], res["u"], res["c"])
        bq = R.bound_same(x16.float(), x16.abs(), res["wg"].abs(), d, q64, tdt)   # includes one rounding of q
        q16 = q64.to(tdt)
        ref, mag = kq_ref(q16, Wk, H, d)
        carried = torch.einsum("mhi,hic->mhc", (bq + R.EPS[tdt] * q64.abs()).reshape(-1, H, 64), Wk.double().abs().reshape(H, 64, d)).reshape(-1, H * d)
        out = res["out"]
        assert torch.equal(out[M:], torch.full_like(out[M:], SENT)) and torch.isfinite(out[:M].float()).all()
        worst = max(worst, R.ratio(out[:M], ref, 4 * 64 * 2.0 ** -24 * mag + R.rounding(ref, tdt) + carried))
    assert worst < 1.0, worst
    report(f"xqk {pname} nch{nch} {dt} d={d}", acc=worst)


def test_undefined_combinations_are_refused():
    """Every (kind, path) pair of UNDEFINED returns WCB_ERR_UNSUPPORTED on otherwise valid operands and writes nothing."""
    assert len(UNDEFINED) < 6 * 7 / 4   # under a quarter of the (kind, path) grid
    kinds = dict(LN_KINDS, resid=L.PROJ_RESID, kq=L.PROJ_KQ, xqk=L.PROJ_XQK)
    paths = {**PATHS64, **PATHS_T}
    d, tdt = 768, torch.bfloat16
    for kname, pname in UNDEFINED:
        M = 80 if pname in PATHS_T else 17
        Mp = up(M, 64)
        buf = lambda *s, t=tdt: torch.full(s, SENT, dtype=t, device="cuda")   # noqa: E731
        z = lambda *s, t=torch.float32: torch.zeros(s, dtype=t, device="cuda")   # noqa: E731
        out = buf(Mp, (d // 64) * d)
        kw = dict(ln_w=z(d), ln_b=z(d), W=z(3 * d if kname == "qkv" else d, d, t=tdt), bias=z(3 * d), Wk=z(d, d, t=tdt), x=z(Mp, d),
                  a16=z(Mp, d, t=tdt), a_fm=z(Mp, d, t=tdt) if pname == "foldfm" else 0, out=out, out16=buf(Mp, d), rst_in=z(Mp, d // 32, 2))
        if kname == "qkv":
            kw.update(kv=buf(2, M + 1, d // 64, 8, 64), pos=torch.zeros(1, dtype=torch.int32, device="cuda"), kv_B=M + 1, kv_T=8, n_split=d)
        proj(kinds[kname], paths[pname], "bf16", M, 3 * d if kname == "qkv" else d, d, expect_rc=-4, **kw)
        assert torch.equal(out.cpu(), torch.full_like(out.cpu(), SENT))


# ------------------------------------------------------------------------------------------------ the step embedding
def embed(dt, tok, pemb, ids, pos, M, d, rps, *, pos_off=None, st_w=0, want16=True, want_fm=False):
    lib, tdt = L.load(), DT[dt][0]
    Mp = up(M, 64)
    x = torch.full((Mp, d), SENT, device="cuda")
    x16 = torch.full((Mp, d), SENT, dtype=tdt, device="cuda") if want16 else None
    xfm = torch.full((Mp * d,), float("nan"), dtype=tdt, device="cuda") if want_fm else None
    st = torch.full((Mp, d // st_w, 2), SENT, device="cuda") if st_w else None
    keep = [tok.cuda(), pemb.cuda(), torch.tensor(ids, dtype=torch.int32, device="cuda"), torch.tensor([pos], dtype=torch.int32, device="cuda"),
            torch.tensor(pos_off, dtype=torch.int32, device="cuda") if pos_off is not None else None]
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = lib.wcb_op_embed(DT[dt][1], *[ptr(t) for t in keep], M, d, tok.shape[0], pemb.shape[0], rps, ptr(x), ptr(x16), ptr(xfm),
                          ptr(st), st_w or 16, _s())
    sync(rc)
    assert rc == 0, (rc, lib.wcb_last_error(None))
    return dict(x=x, x16=x16, xfm=xfm, st=st)


def embed_ref(tok, pemb, ids, pos, rps, pos_off=None):
    V, n_pos = tok.shape[0], pemb.shape[0]
    rows = []
    for r, i in enumerate(ids):
        p = pos + r % rps
        if pos_off is not None:
            p = max(min(p - pos_off[r // rps], n_pos - 1), 0)
        rows.append(tok[i if 0 <= i < V else 0].float() + pemb[p].float())   # one f32 add of two 16-bit values
    return torch.stack(rows)


def embed_tables(seed, V, n_pos, d, tdt):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randn(V, d, generator=g).to(tdt)
    pemb = (torch.randn(n_pos, d, generator=g) * 0.5 + 4.0).to(tdt)   # rows of mean 4: not centred
    return tok, pemb, g


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("rps", [1, 3])
@pytest.mark.parametrize("d", [64, 384, 768, 1280])
@pytest.mark.parametrize("ragged", [False, True])
def test_embed(d, rps, dt, ragged):
    tdt = DT[dt][0]
    V, n_pos = 50, 12
    M = 37 if rps == 1 else 36   # (rows are (sequence, position) pairs: 12 sequences of 3)
    tok, pemb, g = embed_tables(d + rps, V, n_pos, d, tdt)
    ids = torch.randint(0, V, (M,), generator=g).tolist()
    ids[3], ids[M - 1], ids[7] = -1, V, V + 1000          # out of range: row 0
    pos = 9 if ragged else 5
    # ragged: a slot before its prompt (offset > slot: clamped to position 0) and positions clamped at n_pos − 1
    pos_off = [((0, 11, 2, -5)[s % 4]) for s in range(M // rps)] if ragged else None
    fm_ok = dt != "f32" and d in R.LEAN_CFG
    for st_w in (16, 32):
        def run():
            return embed(dt, tok, pemb, ids, pos, M, d, rps, pos_off=pos_off, st_w=st_w, want_fm=fm_ok)
        a, b = run(), run()
        for k in a:
            if a[k] is not None:
                assert torch.equal(bits(a[k]), bits(b[k])), k
        ref = embed_ref(tok, pemb, ids, pos, rps, pos_off)
        x = a["x"].cpu()
        assert torch.equal(x[:M], ref), "x is not exact"
        assert torch.equal(x[M:], torch.full_like(x[M:], SENT))
        assert torch.equal(bits(a["x16"].cpu()[:M]), bits(ref.to(tdt))), "x16 is not T(x)"
        stats_check(a["st"].cpu(), ref, st_w, M)
        if fm_ok:
            nw, kpw = R.LEAN_CFG[d]
            flat = a["xfm"].cpu()
            want = torch.full_like(flat, float("nan"))
            r = torch.arange(M)[:, None].expand(M, d)
            c = torch.arange(d)[None, :].expand(M, d)
            want[R.frag_index(r, c, nw, kpw).reshape(-1)] = ref.to(tdt).reshape(-1)
            assert torch.equal(bits(flat), bits(want)), "fragment-major copy"


def test_embed_refuses_a_fragment_major_copy_it_cannot_write():
    tok, pemb, _ = embed_tables(1, 8, 4, 384, torch.bfloat16)
    lib = L.load()
    buf = torch.zeros(16 * 384, device="cuda")
    t = [tok.cuda(), pemb.cuda(), torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")]
    rc = lib.wcb_op_embed(L.WCB_BF16, *[v.data_ptr() for v in t], None, 4, 384, 8, 4, 1, buf.data_ptr(), None, buf.data_ptr(), None, 16, _s())
    assert rc == -4   # d = 384 is not in the lean table


# ------------------------------------------------------------------------------------------------ chains
CHAIN_MS = [5, 17, 48]


def chain_x(dt, M, d, st_w, want_fm):
    """embedding rows for M tokens at position 2 (one position per row) -> device outputs + the exact f32 rows."""
    tdt = DT[dt][0]
    tok, pemb, g = embed_tables(M + d, 64, 8, d, tdt)
    ids = torch.randint(0, 64, (M,), generator=g).tolist()
    e = embed(dt, tok, pemb, ids, 2, M, d, 1, st_w=st_w, want_fm=want_fm)
    ref = embed_ref(tok, pemb, ids, 2, 1)
    assert torch.equal(e["x"].cpu()[:M], ref)
    return e, ref


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", CHAIN_MS + [70, 320])
def test_chain_embed_to_qkv(M, dt):
    """(a) wcb_op_embed's x16fm (<= 64 rows: lean, folded, fragment-major) or its x16 + 32-column statistics (> 64 rows:
    folded ring tile) straight into the QKV launch; the end against fp64 of the embedding rows."""
    d, tdt = 768, DT[dt][0]
    N = 3 * d
    gam, bet, W, bias = R.make_weights(d + M, N, d, tdt)
    e, x = chain_x(dt, M, d, 32, M <= 64)
    pname = "foldfm" if M <= 64 else "ringfold"
    path = {**PATHS64, **PATHS_T}[pname]
    x16 = e["x16"].cpu()[:M]
    res = twice(lambda: ln_launch(L.PROJ_QKV, path, dt, M, N, d, x, gam, bet, W, bias, pos=3, a_fm=e["xfm"], x16=x16, rst=e["st"]))
    assert res["taken"] & 255 == WANT[pname]
    rs, rt = ln_check(f"chain-a/{dt}/M{M}", L.PROJ_QKV, pname, dt, M, N, d, x, gam, bet, W, bias, res, pos=3, x16=x16, special=False)
    report(f"chain embed->qkv {pname} {dt} M={M}", same=rs, true=rt)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", CHAIN_MS + [70, 320])
def test_chain_resid_to_fc1(M, dt):
    """(b) a residual writer's out16_fm (<= 64 rows) or out16 + rst_out (> 64 rows) into the LN-fused GELU launch."""
    d, F, tdt = 768, 2048, DT[dt][0]
    A, Wo, bo, x0 = resid_inputs(M * 3 + 1, M, d, d, tdt)
    gam, bet, W1, b1 = R.make_weights(M + 9, F, d, tdt)
    lean = M <= 64
    r = resid_launch(L.PATH_LEAN_FOLD_FM if lean else L.PATH_RING_FOLD, dt, M, d, d, A, Wo, bo, x0, want_fm=lean, rst32=not lean)
    resid_check("chain-b/resid", dt, M, d, d, A, Wo, bo, x0, r)
    x, x16 = r["x"][:M], r["out16"][:M]
    pname = "foldfm" if lean else "ringfold"
    path = {**PATHS64, **PATHS_T}[pname]
    a_fm = r["out16_fm"].cuda() if lean else None
    rst = r["rst_out"].cuda() if not lean else None
    res = twice(lambda: ln_launch(L.PROJ_LN_GELU, path, dt, M, F, d, x, gam, bet, W1, b1, a_fm=a_fm, x16=x16, rst=rst))
    assert res["taken"] & 255 == WANT[pname]
    rs, rt = ln_check(f"chain-b/{dt}/M{M}", L.PROJ_LN_GELU, pname, dt, M, F, d, x, gam, bet, W1, b1, res, x16=x16, special=False)
    report(f"chain resid->fc1 {pname} {dt} M={M}", same=rs, true=rt)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("d,F", [(512, 2048), (768, 3072), (1280, 5120)])
@pytest.mark.parametrize("M", CHAIN_MS)
def test_chain_fc1_to_fc2(M, d, F, dt):
    """(c) fc1 writes its GELU output fragment-major in fc2's split of K = ffn; fc2 reads it: the end against fp64 of
    fc2 on fc1's own (checked) 16-bit output."""
    tdt = DT[dt][0]
    gam, bet, W1, b1 = R.make_weights(d + F, F, d, tdt)
    x = R.make_rows(d + M, M, d, 4, 1)
    nw, kpw = R.LEAN_CFG[d]
    Mp = up(M, 64)
    a_fm = R.frag_pack(pad(x.to(tdt), Mp, float("nan")).cpu(), nw, kpw).cuda()
    tdt_out = torch.full((Mp * F,), float("nan"), dtype=tdt, device="cuda")
    kw = dict(ln_w=gam.cuda(), ln_b=bet.cuda(), W=W1.cuda(), bias=b1.cuda(), x=pad(x, Mp, float("nan")), a_fm=a_fm, out=tdt_out, out_fm=1,
              u_out=torch.empty(F, device="cuda"), c_out=torch.empty(F, device="cuda"), wg_out=torch.empty(F, d, dtype=tdt, device="cuda"))
    assert proj(L.PROJ_LN_GELU, L.PATH_LEAN_FOLD_FM, dt, M, F, d, **kw) == L.TAKEN_LEAN
    nw2, kpw2 = R.LEAN_CFG[F]
    h = R.frag_unpack(tdt_out.cpu().reshape(Mp // 16, nw2, kpw2, 64, 8), Mp, F)
    assert torch.isnan(h[M:].float()).all(), "a padded row of the fragment-major output was written"
    res1 = dict(out=torch.cat([h[:M], torch.full((Mp - M, F), SENT, dtype=tdt)]), taken=L.TAKEN_LEAN, u_out=kw["u_out"].cpu(),
                c_out=kw["c_out"].cpu(), wg_out=kw["wg_out"].cpu())
    rs, rt = ln_check(f"chain-c/fc1/{dt}", L.PROJ_LN_GELU, "foldfm", dt, M, F, d, x, gam, bet, W1, b1, res1)
    g = torch.Generator().manual_seed(M + F)
    W2 = (torch.randn(d, F, generator=g) / F ** 0.5).to(tdt)
    b2 = torch.randn(d, generator=g).float()
    res = twice(lambda: resid_launch(L.PATH_LEAN_FOLD_FM, dt, M, d, F, None, W2, b2, x, a_fm=tdt_out, want_fm=True))
    assert res["taken"] == L.TAKEN_LEAN
    acc = resid_check(f"chain-c/fc2/{dt}", dt, M, d, F, h[:M], W2, b2, x, res)
    report(f"chain fc1->fc2 {dt} M={M} d={d}", same=rs, true=rt, acc=acc)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M", CHAIN_MS)
def test_chain_legacy_statistics_to_gemm_ln(M, dt):
    """(d) the 16-column statistics of wcb_op_embed (st_w = 16) and of a residual writer (st_out) into wcb_op_gemm_ln,
    K = 384. At this width the decode GEMM recomputes the row statistics from the rows it loads, so the partials are
    also held to fp64 sums directly (stats_check)."""
    lib, tdt = L.load(), DT[dt][0]
    K, N = 384, 192
    gam, bet, W, bias = R.make_weights(M + K, N, K, tdt)
    e, x_emb = chain_x(dt, M, K, 16, False)
    stats_check(e["st"].cpu(), x_emb, 16, M)
    A, Wo, bo, _ = resid_inputs(M + 2, M, K, K, tdt)
    r = resid_launch(L.PATH_DEC, dt, M, K, K, A, Wo, bo, x_emb, st16=True)
    assert r["taken"] == L.TAKEN_DEC_MF
    resid_check("chain-d/resid", dt, M, K, K, A, Wo, bo, x_emb, r)
    gam_d, bet_d, W_d, bias_d = gam.cuda(), bet.cuda(), W.cuda(), bias.cuda()   # (kept alive across the calls)
    for x, st in ((x_emb, e["st"]), (r["x"][:M], r["st_out"].cuda())):
        xd = pad(x, up(M, 64), float("nan"))
        outs = []
        for _ in range(2):
            out = torch.full((up(M, 64), N), SENT, device="cuda")
            L.check(lib.wcb_op_gemm_ln(DT[dt][1], xd.data_ptr(), gam_d.data_ptr(), bet_d.data_ptr(), st.data_ptr(),
                                       W_d.data_ptr(), M, N, K, bias_d.data_ptr(), 0, out.data_ptr(), 1, _s()))
            sync()
            outs.append(out.cpu())
        assert torch.equal(bits(outs[0]), bits(outs[1]))
        out = outs[0]
        assert torch.equal(out[M:], torch.full_like(out[M:], SENT)) and torch.isfinite(out[:M]).all()
        true = R.ref_true(x, gam, bet, W, bias)
        if dt == "f32":   # f32 LayerNorm and product: K·2^-24 relative to r·Σ|x||γW| + |ref|
            _, rr = R.stats64(x)
            bound = 4 * K * 2.0 ** -24 * (rr * (x.double().abs() @ (gam.double().abs()[None] * W.double().abs()).T) + true.abs())
        else:
            bound = R.bound_true(x, gam, W, true, tdt)
        ratio = R.ratio(out[:M], true, bound)
        assert ratio < 1.0, ratio
        report(f"chain stats16->gemm_ln {dt} M={M}", true=ratio)
