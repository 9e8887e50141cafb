"""The parallel branch head's kernels against fp64: the CLS pooling kernels (csrc/clspool.hip: sc_cls_scores, sc_cls_pool_fwd,
sc_cls_pool_bwd) at every template instance, with the train-mode arguments, the length clamp, poisoned padding and the host-side
refusals; every entry point of csrc/rowtail.hip at one row, fewer than eight rows and across 64-row tiles; the whole head
(head_tail.ParallelHeadFn, with cls_query on csrc/headtail.hip) at the base and large recipe widths.

Inputs, references and bounds come from tests/head_cases.py (seeded; fp64 references, the backward by autograd on the fp64 forward;
the same functions in fp32 on the CPU are the yardstick).  The error is taken per row of a quantity's natural grouping.  Bounds
(docs/parity.md, "Parallel head"): sums and dot products ``k u sum |a_i b_i|`` per output with k from the launch geometry;
quantities through exp, rsqrt, division or GELU ``max(4 x the yardstick's error on the case, 2^-23)``; the dX row of a key that the
dropout drops may meet its own derived bound instead (it holds -p dot a, the relative error of a cancelling sum: 8.3e-7 against a
yardstick of 1.6e-7 at (64, 1, 40), p = 0.1, where dot cancels 31 : 1).  Every figure is printed as a
``PARITY|case|quantity|error|yardstick|bound`` line before anything is asserted, and a test fails once with all its violations."""
import ctypes

import pytest
import torch

import head_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _ops():
    from speechclip_plus_amd import ops
    return ops


def _run_pool(dev, c, inp, mult=None, cbias=None, dp_preformed=False):
    """The three kernels on a case's inputs -> the quantities of head_cases.POOL_DIMS (da = sum_b da_part, added in fp64)."""
    ops = _ops()
    B, R, D, H = c["B"], c["R"], c["D"], c["H"]
    X = c["X"].to(torch.bfloat16).to(dev)
    assert torch.equal(X.float().cpu(), c["X"])
    a, dm, lens = c["a"].to(dev), c["dm"].to(dev).contiguous(), c["lens"].to(dev)
    got = {"scores": ops.cls_scores(X, a, False, B, R, D, H), "dp": ops.cls_scores(X, dm, True, B, R, D, H)}
    md = mult.to(dev) if mult is not None else None
    if md is not None:
        got["p"], got["m"], got["psum"] = ops.cls_pool_fwd(X, inp["scores"].to(dev), lens, B, R, D, H, md, want_psum=True)
    else:
        got["p"], got["m"] = ops.cls_pool_fwd(X, inp["scores"].to(dev), lens, B, R, D, H)
    dp = inp["dp"].to(dev)
    if dp_preformed:                                      # the caller's convention: dp = (dp + cbias) mult, formed in fp32 as the kernel does
        dp = ((dp + cbias.to(dev)[..., None]) * md).contiguous()
        got["dX"], da_part = ops.cls_pool_bwd(X, inp["p"].to(dev), dp, dm, a, lens, B, R, D, H, md, cbias=None)
    else:
        got["dX"], da_part = ops.cls_pool_bwd(X, inp["p"].to(dev), dp, dm, a, lens, B, R, D, H, md,
                                              cbias=cbias.to(dev) if cbias is not None else None)
    got["da_part"] = da_part
    got["da"] = da_part.double().sum(0)
    return got


def _quantities(got):
    return {k: v for k, v in got.items() if k in hc.POOL_DIMS}


# ---------------------------------------------------------------------------------------------------------------- (a) shape sweep
@pytest.mark.parametrize("D,H,R", hc.POOL_SWEEP)
def test_pool_shape_sweep(dev, D, H, R):
    """NCH 1 .. 4, every NH instance (H = 16: two passes of eight heads in the scores), R below one wave's 16 rows, R off every
    multiple of 8 / 16 / 32 / 64, a clamped last score block; lengths [R, 1, no multiple of 32, R // 2 + 1]; the shared ``a``
    (per_batch = False) and the per-utterance dm sweep (per_batch = True).  Every D of the sweep is a multiple of 64 (320 = 5 x 64), so
    all three kernels run in every case."""
    c = hc.pool_case(D, H, R)
    ref, inp = hc.pool_reference(c)
    yard, bounds = hc.pool_yardstick(c, inp), hc.pool_bounds(c, inp)
    got = _run_pool(dev, c, inp)
    rep = hc.Report()
    hc.pool_checks(rep, f"sweep D={D} H={H} R={R}", c, _quantities(got), ref, yard, bounds)
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- (b) train mode
@pytest.mark.parametrize("p_drop", hc.TRAIN_P)
@pytest.mark.parametrize("D,H,R", hc.TRAIN_CASES)
def test_pool_train_mode_arguments(dev, D, H, R, p_drop):
    """mult / psum / cbias: p stays un-masked, m and psum use p mult; the backward in both conventions (cbias given with the raw dp;
    cbias = None with dp pre-formed as (dp + cbias) mult) against autograd through ctx_h = Wv_h (sum p mult X) + bv_h sum p mult.
    The two conventions evaluate the same fp32 expression - the kernel forms (dp + cbias) * mult as one addition and one product, no
    fused form exists for that order - so their results agree to the bit."""
    c = hc.train_case(D, H, R, p_drop)
    mult, cbias = c["mult"], c["cbias"]
    ref, inp = hc.pool_reference(c, mult, cbias)
    yard, bounds = hc.pool_yardstick(c, inp, mult, cbias), hc.pool_bounds(c, inp, mult, cbias)
    name = f"train D={D} H={H} R={R} p={p_drop}"
    rep = hc.Report()
    got = _run_pool(dev, c, inp, mult, cbias)
    hc.pool_checks(rep, name + " cbias", c, _quantities(got), ref, yard, bounds, mult)
    got2 = _run_pool(dev, c, inp, mult, cbias, dp_preformed=True)
    hc.pool_checks(rep, name + " preformed", c, {k: got2[k] for k in ("dX", "da")}, ref, yard, bounds, mult)
    rep.equal(name, "dX, cbias given vs dp pre-formed", got["dX"], got2["dX"])
    rep.equal(name, "da_part, cbias given vs dp pre-formed", got["da_part"], got2["da_part"])
    # p is the softmax itself: the same bits as the run without multipliers
    plain = _run_pool(dev, c, inp)
    rep.equal(name, "p with and without mult", got["p"], plain["p"])
    rep.done()


@pytest.mark.parametrize("B,D,H", hc.VALUE_BIAS_CASES)
def test_value_bias_bwd(dev, B, D, H):
    """sc_rt_value_bias_bwd: cbias[b, h] = dctx_h . bv_h (dh = 64, 96, 128, 768) and gbv += sum_b dctx psum on top of non-zero
    contents (D above one 256-column block, B above one 64-row tile)."""
    c = hc.value_bias_case(B, D, H)
    ref, yard, bounds = hc.value_bias_ref(c, torch.float64), hc.value_bias_ref(c, torch.float32), hc.value_bias_bounds(c)
    gbv = c["gbv0"].to(dev).clone()
    cb = _ops().rt_value_bias_bwd(c["dctx"].to(dev), c["bv"].to(dev), c["psum"].to(dev), gbv, H)
    rep = hc.Report()
    name = f"value_bias B={B} D={D} H={H}"
    rep.derived(name, "cbias", cb, ref["cbias"], bounds["cbias"], (), yard["cbias"])
    v = lambda t: t.view(H, D // H)
    rep.derived(name, "gbv", v(gbv), v(ref["gbv"]), v(bounds["gbv"]), (1,), v(yard["gbv"]))
    rep.done()


@pytest.mark.parametrize("nblk,NL", hc.SOFTMAX_REDUCE_CASES)
def test_softmax_bwd_reduce(dev, nblk, NL):
    """sc_rt_softmax_bwd_reduce: the column sums of the [nblk, NL] partials (below, at and above one 256-thread pass) and the softmax
    backward on them.  NL = 1: w = 1 and the result is exactly zero."""
    from speechclip_plus_amd._lib import check, lib
    ops = _ops()
    part, w = hc.softmax_reduce_case(nblk, NL)
    out = torch.full((NL,), float("nan"), device=dev)
    pd, wd = part.to(dev), w.to(dev)
    check(lib().sc_rt_softmax_bwd_reduce(ops._p(pd), nblk, NL, ops._p(wd), ops._p(out), ops._stream()), "sc_rt_softmax_bwd_reduce")
    rep = hc.Report()
    rep.derived(f"softmax_reduce nblk={nblk} NL={NL}", "out", out, hc.softmax_reduce_ref(part.double(), w.double()),
                hc.softmax_reduce_bound(part, w), (0,), hc.softmax_reduce_ref(part, w))
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- (c) clamp, padding, refusals
def _pool_all(dev, c, X, lens, scores=None):
    """scores -> pool forward (with mult and psum) -> dp -> pool backward (cbias), chained on the device as the head does."""
    ops = _ops()
    B, R, D, H = c["B"], c["R"], c["D"], c["H"]
    a, dm, mult, cbias = c["a"].to(dev), c["dm"].to(dev).contiguous(), c["mult"].to(dev), c["cbias"].to(dev)
    s = ops.cls_scores(X, a, False, B, R, D, H) if scores is None else scores
    p, m, psum = ops.cls_pool_fwd(X, s, lens, B, R, D, H, mult, want_psum=True)
    dp = ops.cls_scores(X, dm, True, B, R, D, H)
    dX, da = ops.cls_pool_bwd(X, p, dp, dm, a, lens, B, R, D, H, mult, cbias=cbias)
    return {"p": p, "m": m, "psum": psum, "dX": dX, "da_part": da}


def test_pool_length_clamp(dev):
    """n = max(1, min(len, R)): len = 0 and -3 give the bits of len = 1, len = R + 5 the bits of len = R."""
    c = hc.train_case(768, 8, 320, 0.1)
    R = c["R"]
    X = c["X"].to(torch.bfloat16).to(dev)
    L = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)
    base = _pool_all(dev, c, X, L(1, 1, R, R))
    odd = _pool_all(dev, c, X, L(0, -3, R + 5, R))
    rep = hc.Report()
    for k in base:
        rep.equal("length clamp", k, base[k], odd[k])
    rep.done()


def test_pool_poisoned_padding_rows(dev):
    """Rows s >= len of X filled with NaN and +-Inf bf16 patterns: p, m, psum and da_part keep the bits of the run on zero padding,
    p and dX are exactly 0 on s >= n, dX is finite on s < n; two runs give the same bits.  (The scores of padded rows may be
    anything: sc_cls_scores reads them on purpose and its consumers ignore them.)"""
    c = hc.train_case(768, 8, 320, 0.1)
    B, R, D = c["B"], c["R"], c["D"]
    lens = c["lens"].to(dev)
    X0 = c["X"].to(torch.bfloat16).to(dev)
    dead = ~hc.live_mask(c["lens"], R).to(dev)
    poison = torch.tensor([0x7FC0, 0x7F80, 0xFF80, 0xFFC1], dtype=torch.int32)[torch.arange(B * R * D) % 4].to(torch.int16)
    Xp = torch.where(dead[..., None], poison.view(B, R, D).to(dev).view(torch.bfloat16), X0).contiguous()
    assert not bool(torch.isfinite(Xp.float()[dead]).any()) and torch.equal(Xp[~dead], X0[~dead])
    clean, dirty, again = _pool_all(dev, c, X0, lens), _pool_all(dev, c, Xp, lens), _pool_all(dev, c, Xp, lens)
    rep = hc.Report()
    for k in ("p", "m", "psum", "da_part"):
        rep.equal("poisoned padding", k + " against zero padding", clean[k], dirty[k])
    for k in clean:
        rep.equal("poisoned padding", k + " repeated", dirty[k], again[k])
    rep.require("poisoned padding", "p != 0 on s >= n", bool((dirty["p"][dead[:, None, :].expand_as(dirty["p"])] == 0).all()))
    rep.require("poisoned padding", "dX != 0 on s >= n", bool((dirty["dX"][dead] == 0).all()))
    rep.require("poisoned padding", "dX not finite on s < n", bool(torch.isfinite(dirty["dX"][~dead]).all()))
    rep.equal("poisoned padding", "dX on s < n against zero padding", clean["dX"][~dead], dirty["dX"][~dead])
    rep.done()


SENTINEL = -12345.0


def _raw_fwd(dev, X, B, R, D, H, xptr=None):
    """sc_cls_pool_fwd through the C ABI on sentinel-filled outputs -> (return code, p, m)"""
    from speechclip_plus_amd._lib import lib
    ops = _ops()
    scores = torch.zeros(B, H, R, device=dev)
    lens = torch.full((B,), R, dtype=torch.int32, device=dev)
    p, m = torch.full((B, H, R), SENTINEL, device=dev), torch.full((B, H, D), SENTINEL, device=dev)
    rc = lib().sc_cls_pool_fwd(ops._p(X) if xptr is None else ctypes.c_void_p(xptr), ops._p(scores), ops._p(lens), ops._p(p), ops._p(m),
                               B, R, D, H, None, None, ops._stream())
    torch.cuda.synchronize()
    return rc, p, m


def _raw_bwd(dev, X, B, R, D, H, xptr=None):
    from speechclip_plus_amd._lib import lib
    ops = _ops()
    z = lambda *s: torch.zeros(*s, device=dev)
    lens = torch.full((B,), R, dtype=torch.int32, device=dev)
    dX, da = torch.full((B, R, D), SENTINEL, device=dev), torch.full((B, H, D), SENTINEL, device=dev)
    p, dp, dm, a = z(B, H, R), z(B, H, R), z(B, H, D), z(H, D)
    rc = lib().sc_cls_pool_bwd(ops._p(X) if xptr is None else ctypes.c_void_p(xptr), ops._p(p), ops._p(dp), ops._p(dm), ops._p(a),
                               ops._p(lens), ops._p(dX), ops._p(da), B, R, D, H, None, None, ops._stream())
    torch.cuda.synchronize()
    return rc, dX, da


def _raw_scores(dev, X, B, R, D, H, xptr=None):
    from speechclip_plus_amd._lib import lib
    ops = _ops()
    vec = torch.zeros(H, D, device=dev)
    s = torch.full((B, H, R), SENTINEL, device=dev)
    rc = lib().sc_cls_scores(ops._p(X) if xptr is None else ctypes.c_void_p(xptr), ops._p(vec), 0, ops._p(s), B, R, D, H, ops._stream())
    torch.cuda.synchronize()
    return rc, s


def _untouched(*ts):
    return all(bool((t == SENTINEL).all()) for t in ts)


def test_pool_refusals_are_host_side_and_write_nothing(dev):
    """The 64 KiB LDS checks accept the largest R of the formula in the source (head_cases.pool_lds_limits) and refuse the next
    multiple of 8 with an error that names LDS; H = 3, D = 1028 for the scores, D = 96 for the pool and a misaligned X are refused
    too.  These are argument checks on the host: a refused call launches nothing and leaves sentinel-filled outputs untouched."""
    from speechclip_plus_amd._lib import check
    B, D, H = 1, 64, 8
    r_fwd, r_bwd = hc.pool_lds_limits(H)
    assert H * (r_fwd + 256) * 4 <= hc.LDS_BYTES < H * (r_fwd + 8 + 256) * 4
    assert H * (2 * r_bwd + 256) * 4 <= hc.LDS_BYTES < H * (2 * (r_bwd + 8) + 256) * 4
    bad = []
    X = torch.zeros(B, r_fwd + 8, D, device=dev, dtype=torch.bfloat16)
    # accepted: uniform scores over zero rows -> p = 1 / R, m = 0
    rc, p, m = _raw_fwd(dev, X[:, :r_fwd].contiguous(), B, r_fwd, D, H)
    check(rc, "sc_cls_pool_fwd")
    if not (torch.allclose(p, torch.full_like(p, 1.0 / r_fwd), rtol=1e-6) and bool((m == 0).all())):
        bad.append(f"forward at R = {r_fwd}: wrong result")
    rc, dX, da = _raw_bwd(dev, X[:, :r_bwd].contiguous(), B, r_bwd, D, H)
    check(rc, "sc_cls_pool_bwd")
    if not (bool((dX == 0).all()) and bool((da == 0).all())):
        bad.append(f"backward at R = {r_bwd}: wrong result")
    # refused
    rc, p, m = _raw_fwd(dev, X, B, r_fwd + 8, D, H)
    with pytest.raises(RuntimeError, match="LDS"):
        check(rc, "sc_cls_pool_fwd")
    if not _untouched(p, m):
        bad.append("refused forward (LDS) wrote its outputs")
    rc, dX, da = _raw_bwd(dev, X[:, :r_bwd + 8].contiguous(), B, r_bwd + 8, D, H)
    with pytest.raises(RuntimeError, match="LDS"):
        check(rc, "sc_cls_pool_bwd")
    if not _untouched(dX, da):
        bad.append("refused backward (LDS) wrote its outputs")
    R = 16
    for what, fn, args, msg in [("H = 3 scores", _raw_scores, (B, R, 192, 3), "H=3 not in"), ("H = 3 forward", _raw_fwd, (B, R, 192, 3), "H=3 not in"),
                                ("H = 3 backward", _raw_bwd, (B, R, 192, 3), "H=3 not in"),
                                ("D = 1028 scores", _raw_scores, (B, R, 1028, 4), "<= 1024"),
                                ("D = 96 forward", _raw_fwd, (B, R, 96, 1), "D % 64"), ("D = 96 backward", _raw_bwd, (B, R, 96, 1), "D % 64")]:
        Bq, Rq, Dq, Hq = args
        rc, *outs = fn(dev, torch.zeros(Bq, Rq, Dq, device=dev, dtype=torch.bfloat16), *args)
        with pytest.raises(RuntimeError, match=msg):
            check(rc, what)
        if not _untouched(*outs):
            bad.append(f"refused call ({what}) wrote its outputs")
    # a misaligned X: one bf16 element past a 16-byte boundary
    buf = torch.zeros(B * R * D + 8, device=dev, dtype=torch.bfloat16)
    assert buf.data_ptr() % 16 == 0
    for what, fn in [("misaligned scores", _raw_scores), ("misaligned forward", _raw_fwd), ("misaligned backward", _raw_bwd)]:
        rc, *outs = fn(dev, buf, B, R, D, H, xptr=buf.data_ptr() + 2)
        with pytest.raises(RuntimeError, match="align"):
            check(rc, what)
        if not _untouched(*outs):
            bad.append(f"refused call ({what}) wrote its outputs")
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- (d) row tail
class _ForcedSlices:
    """The library with sc_rt_gemm_slices answering a fixed S: ops.rt_gemm(split=True) then splits the contraction that way."""

    def __init__(self, real, S):
        self._real, self._S = real, S

    def __getattr__(self, name):
        return getattr(self._real, name)

    def sc_rt_gemm_slices(self, *args):
        return self._S


def _run_tail(dev, c, inp):
    """Every row-tail operation on a case's host-made inputs -> (the quantities of head_cases.tail_reference, the slice counts)."""
    ops = _ops()
    d = lambda k: c[k].to(dev).contiguous()
    B, D, F_, E, H, dh = c["B"], c["D"], c["F"], c["E"], c["H"], c["dh"]
    x, W1, b1 = d("x"), d("W1"), d("b1")
    got, S = {}, {}
    ys = ops.rt_gemm(x, W1, B, F_, D, split=True)
    got["gemm_split"], S["x_W1"] = ys.total(), ys.ns
    C, Um = d("C0").clone(), torch.empty(B, F_, device=dev)
    ops.rt_gemm(x, W1, B, F_, D, out=C, alpha=0.5, beta=2.0, bias=b1, act=1, U=Um, drop_p=hc.P_F, drop_seed=hc.SEED_F)
    got["gemm_U"], got["gemm_C"] = Um, C
    ysl, rs = ops.Slices(d("ysl")), d("rs")
    got["elem0"] = ops.rt_elem(ysl, 0, bias=b1, rowscale=rs, group=F_ // H)
    zs = ops.rt_gemm(ysl, W1, B, D, F_, a_bias=b1, a_rowscale=rs, a_group=F_ // H, b_kmajor=True, ldb=D, split=True)
    got["gemm_sliced"], S["sliced"] = zs.total(), zs.ns
    gW, gb = d("gW0").clone(), d("gb0").clone()
    ops.rt_gemm(d("dy"), x, F_, D, B, a_kmajor=True, b_kmajor=True, lda=F_, ldb=D, out=gW, beta=1.0, gb=gb)
    got["gW"], got["gb"] = gW, gb
    m, Wv, dc = d("m"), d("Wv"), d("dc")
    cs = ops.rt_gemm(m, Wv, B, dh, D, nbatch=H, lda=H * D, a_z=D, ldb=D, b_z=dh * D, split=True, ldc=D, c_z=dh)
    got["h_ctx"], S["ctx"] = cs.total(), cs.ns
    gWv, gbv = d("gWv0").clone(), d("gbv0").clone()
    ops.rt_gemm(dc, m, dh, D, B, a_kmajor=True, b_kmajor=True, lda=D, ldb=H * D, nbatch=H, a_z=dh, b_z=D, out=gWv, ldc=D, c_z=dh * D,
                beta=1.0, gb=gbv, gb_z=dh)
    got["h_gWv"], got["h_gbv"] = gWv, gbv
    dm = torch.empty(B, H, D, device=dev)
    ops.rt_gemm(dc, Wv, B, D, dh, nbatch=H, lda=D, a_z=dh, b_kmajor=True, ldb=D, b_z=dh * D, out=dm, ldc=H * D, c_z=D)
    got["h_dm"] = dm.view(B, H * D)
    zsl, g1, be1, g2, be2 = ops.Slices(d("zsl")), d("g1"), d("be1"), d("g2"), d("be2")
    got["ln1_out"], got["ln1_xhat"], got["ln1_rstd"] = ops.rt_ln_fwd(zsl, d("bias_d"), d("res0"), 0, g1, be1, 1e-5, drop_p=hc.P_D,
                                                                      drop_seed=hc.SEED_D)
    o1, _, _, o2, h2, r2 = ops.rt_ln_fwd(zsl, d("bias_d"), d("resB"), D, g1, be1, 1e-5, g2, be2, 1e-6, drop_p=hc.P_D, drop_seed=hc.SEED_D)
    got["lnc_out1"], got["lnc_out2"], got["lnc_xhat2"], got["lnc_rstd2"] = o1, o2, h2, r2
    dgam, dbet = d("dgam0").clone(), d("dbet0").clone()
    got["lnb_dx"], got["lnb_dxm"] = ops.rt_ln_bwd(ops.Slices(d("dys")), d("add"), inp["xhat"].to(dev), g1, inp["rstd"].to(dev), dgam, dbet,
                                                  want_masked=True, drop_p=hc.P_D, drop_seed=hc.SEED_D)
    got["lnb_dgamma"], got["lnb_dbeta"] = dgam, dbet
    got["elem1_u"], got["elem1_f"] = ops.rt_elem(ysl, 1, bias=b1, drop_p=hc.P_F, drop_seed=hc.SEED_F)
    got["elem2"] = ops.rt_elem(ysl, 2, u=inp["u"].to(dev), drop_p=hc.P_F, drop_seed=hc.SEED_F)
    got["l2_x"], got["l2_e"], got["l2_rn"] = ops.rt_l2norm_fwd(ops.Slices(d("wsl")), d("bp"))
    got["l2_bwd"] = ops.rt_l2norm_bwd(d("ge"), inp["e"].to(dev), inp["rn"].to(dev))
    return got, S


@pytest.mark.parametrize("B,D,F_,E", hc.TAIL_CASES)
def test_rowtail_sweep(dev, monkeypatch, B, D, F_, E):
    """csrc/rowtail.hip per row against fp64 at one row, fewer rows than rt_ln_bwd's 8 column-part groups, and M across one and two
    64-row tiles: rt_gemm split (the S the library picks, then S = 8 forced) and un-split (alpha, bias, GELU with U, dropout, beta),
    the Slices A operand with a_bias / a_rowscale / a_group, the weight-gradient form with gb at beta = 1, the three per-head
    batched forms; rt_ln_fwd single and chained, rt_ln_bwd with add, want_masked, dropout at p = 0.1 and dgamma / dbeta onto
    non-zero contents; rt_elem modes 0 / 1 / 2; rt_l2norm_fwd / _bwd.  Every kernel runs on host-made inputs."""
    ops = _ops()
    c = hc.tail_case(B, D, F_, E)
    ref, inp = hc.tail_reference(c, torch.float64)
    yard = hc.tail_reference(c, torch.float32, inp)
    rep = hc.Report()
    name = f"tail B={B} D={D} F={F_} E={E}"
    got, S = _run_tail(dev, c, inp)
    hc.tail_checks(rep, name, got, ref, yard, hc.tail_bounds(c, inp, S))
    rep.require(name, f"the split products are not split: {S}", S["x_W1"] > 1 and S["sliced"] > 1 and S["ctx"] > 1)
    # S = 8 where the entry allows it (Kc (S - 1) < K): every split product of the case, K = D and K = F
    real = ops.lib()
    monkeypatch.setattr(ops, "lib", lambda: _ForcedSlices(real, 8))
    got8, S8 = _run_tail(dev, c, inp)
    monkeypatch.undo()
    rep.require(name, f"S = 8 was not taken: {S8}", set(S8.values()) == {8})
    split = ("gemm_split", "gemm_sliced", "h_ctx")
    hc.tail_checks(rep, name + " S=8", {k: got8[k] for k in split}, ref, yard, hc.tail_bounds(c, inp, S8))
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- (e) whole head
def _branch(dev, d_model, nhead, ffn, E, W, train):
    from speechclip_plus_amd import Config, KW_ParallelBranch
    cfg = Config({"model_settings": {"parallel_branch": {
        "transformer_type": "TransformerEncoder",
        "transformer_args": {"n_layers": 1, "d_model": d_model, "nhead": nhead, "dim_feedforward": ffn, "dropout": hc.HEAD_P,
                             "activation": "gelu", "layer_norm_eps": 1e-5, "batch_first": True, "norm_first": False},
        "need_projection": True}}})
    br = KW_ParallelBranch(cfg, audio_dim=d_model, text_dim=E).to(dev)
    br.load_state_dict({k: v.clone() for k, v in W.items()}, strict=True)
    return br.train() if train else br.eval()


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("d_model,nhead,ffn,E", hc.HEAD_CASES)
def test_whole_head_at_recipe_widths(dev, d_model, nhead, ffn, E, train):
    """KW_ParallelBranch on ParallelHeadFn (cls_query on csrc/headtail.hip, the pooling kernels, the row tail) at the base and large
    recipe widths, B = 3, T = 100, lengths [100, 37, 1], against oracle.parallel_branch_forward in fp64 under autograd on the
    bf16-valued features: the output per utterance, d feat per frame, d cls and every parameter gradient, each within 4 x the fp32
    oracle's own error on the case.  Train mode (p = 0.1) replays the four masks from the call counter as
    test_parallel_branch_train_mode_dropout_vs_oracle does.  The in_proj_bias key part has an exactly zero reference: |grad| < 1e-4
    of the bias gradient's scale."""
    ops = _ops()
    W = hc.head_weights(d_model, ffn, E)
    feat, lens, gout = hc.head_inputs(d_model, E)
    br = _branch(dev, d_model, nhead, ffn, E, W, train)
    f = feat.to(dev).requires_grad_(True)
    torch.manual_seed(77)
    calls0 = ops._mult_calls[0]
    out = br(audio_feat=f, audio_feat_len=lens.to(dev))["parallel_audio_feat"]
    (out * gout.to(dev)).sum().backward()
    drop = None
    if train:
        ops._mult_calls[0] = calls0
        mk = lambda *shape: ops.dropout_mult(shape, hc.HEAD_P, dev).cpu()
        masks = mk(hc.HEAD_B, nhead, hc.HEAD_R), mk(hc.HEAD_B, d_model), mk(hc.HEAD_B, ffn), mk(hc.HEAD_B, d_model)
        assert 0.8 < float((masks[0] > 0).float().mean()) < 0.97
        drop = hc.head_drop_fn(*masks)
    got = hc.head_quantities(out.detach(), f.grad, {n: p.grad for n, p in br.named_parameters()})
    ref = hc.head_reference(W, feat, lens, gout, nhead, drop)
    yard = hc.head_reference(W, feat, lens, gout, nhead, drop, dtype=torch.float32)
    assert set(got) == set(ref)
    rep = hc.Report()
    name = f"head d={d_model} {'train' if train else 'eval'}"
    hc.head_checks(rep, name, got, ref, yard)
    if train:                                              # the masks matter: the eval output is far away
        ev = hc.head_reference(W, feat, lens, gout, nhead, None)
        rep.require(name, "train mode equals eval mode", hc.rel_l2(ref["out"], ev["out"]) > 0.05)
    dead = ~hc.live_mask(lens.to(torch.int32), hc.HEAD_T)
    rep.require(name, "d feat is not exactly 0 past the length", bool((f.grad.cpu()[dead] == 0).all()))
    rep.done()
