"""A gradient does not depend on the bytes a backward kernel reads but the mathematics excludes (docs/parity.md, "What a kernel reads
and must ignore", subsection "Backward"): K / V / K^T of keys t >= valid_len, q / out / lse2 of pad queries, the scratch a call fills
itself, pad rows of the operand a row-reducing gradient kernel contracts against dy = 0, and memory that nobody wrote.

  (a) sc_attn_bwd_fused_bf16 / sc_attn_bwd_bf16 at the two smallest geometries that reach every branch, plain / dropout / causal: a
      clean run (zeros or the forward's own values under every mask) against runs that give every region the strongest poison its
      class allows -> dq of the rows t < len, dk / dv of the keys t < len carry the bits of the clean run; dk / dv of the keys
      t >= len and dq of every row with dout = 0 are exactly zero; sentinel rows behind the outputs are untouched; the clean run
      itself is held against fp64 with the bounds of tests/attn_cases.py.
  (b) the same kernels with ONE region given more than its class allows: the result then differs - the contract is as weak as
      stated, not weaker.
  (c) sc_attn32_bwd_bf16 and every row-reducing gradient kernel of the trainable encoder at rows = 3 x 128, valid rows 128 / 1 / 37.
  (d) whole train steps (loss and every p.grad): twice, with torch.empty returning NaN on a warm and on a fresh model, and after a
      step on another batch in the same plan.

No tolerance: every assertion is bit equality against a clean run, an exact zero, or a bound tests/attn_cases.py derives."""
import dataclasses

import pytest
import torch

import attn_cases as ac
import poison_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0
SCALE = 0.125
DROP_P, DROP_SEED = 0.1, 20260
_CACHE = {}


def _ops():
    from speechclip_plus_amd import ops
    return ops


def _heads(x, H):
    return x.double().view(x.shape[0], H, 64).transpose(0, 1)


def _all(shape, dtype, patterns):
    """a tensor of ``shape`` holding nothing but the patterns"""
    z = torch.zeros(shape, dtype=dtype)
    m = torch.ones(shape, dtype=torch.bool)
    return pc.poison_bf16(z, m, patterns) if dtype == torch.bfloat16 else pc.poison_f32(z, m, patterns)


# ================================================================================================================== (a) attention backward
def _forward(lay, q, k, v, inst):
    """ops.attn_fwd on q | k and the transposed v (64 rows / elements of zero slack behind them, as tests/test_gpu_poison.py) ->
    out [B R, D] bf16, lse2 [B, H, R] fp32 on the CPU: the forward's own values on EVERY row of the layout"""
    ops = _ops()
    B, R, H, D, rows = lay.B, lay.R, lay.H, lay.D, lay.rows
    qk = torch.zeros(rows + pc.SLACK, 2 * D, dtype=torch.bfloat16)
    qk[:rows] = torch.cat([q, k], dim=1)
    vt = torch.zeros(D * rows + pc.SLACK, dtype=torch.bfloat16)
    vt[: D * rows] = pc.head_transpose(v, lay).reshape(-1)
    out = torch.zeros(rows, D, dtype=torch.bfloat16, device=DEV)
    lse2 = torch.zeros(B, H, R, dtype=torch.float32, device=DEV)
    ops.attn_fwd(qk.to(DEV), vt.to(DEV), torch.tensor(lay.lens, dtype=torch.int32, device=DEV), out, B, R, H, D, SCALE, lse2=lse2,
                 causal=int(inst == "causal"), drop_p=DROP_P if inst == "drop" else 0.0, drop_seed=DROP_SEED)
    torch.cuda.synchronize()
    return out.cpu(), lse2.cpu()


def _case(name, inst):
    """operands of a geometry and the two forwards of an instance - with zeros and with N(0, 64^2) on the q rows t >= len (what a pad
    query is allowed to hold: out and lse2 of such a row must be the forward's own) - built once, shared by both entry points"""
    if name not in _CACHE:
        lay = pc.bwd_case_layout(name)
        _CACHE[name] = (lay, pc.bwd_operands(lay, seed=200 + sorted(pc.BWD_GEOMETRIES).index(name)))
    lay, o = _CACHE[name]
    if (name, inst) not in _CACHE:
        c = dict(o)
        c["out"], c["lse2"] = _forward(lay, o["q"], o["k"], o["v"], inst)
        c["q1"] = pc.put(o["q"], pc.row_mask(~lay.valid, lay.D), o["scratch"])
        c["out1"], c["lse2_1"] = _forward(lay, c["q1"], o["k"], o["v"], inst)
        _CACHE[(name, inst)] = c
    return lay, _CACHE[(name, inst)]


def _backward(entry, lay, inst, t, dirty):
    """one launch of sc_attn_bwd_fused_bf16 (q^T / k^T / dout^T are scratch of the call) or sc_attn_bwd_bf16 (the caller's t["qT"],
    t["kT"], t["doT"]); ``dirty``: delta and the fused entry's scratch hold NaN / Inf on entry instead of zeros.
    -> dq, dk, dv [B R, D] bf16 on the CPU; the 8 sentinel rows behind each are checked here"""
    from speechclip_plus_amd._lib import check, lib
    ops = _ops()
    p = ops._p
    B, R, H, D, rows = lay.B, lay.R, lay.H, lay.D, lay.rows
    assert all(v < R for v in pc.bwd_read_extent(lay).values())
    d = {n: t[n].contiguous().to(DEV) for n in ("q", "k", "v", "out", "dout", "lse2")}
    assert all(tuple(d[n].shape) == (rows, D) for n in ("q", "k", "v", "out", "dout")) and tuple(d["lse2"].shape) == (B, H, R)
    junk = pc.NONFINITE_POISON if dirty else (0,)
    delta = _all((B, H, R), torch.float32, junk).to(DEV)
    if entry == "fused":
        tr = [_all((B, H, 64, R), torch.bfloat16, junk).to(DEV) for _ in range(3)]
    else:
        tr = [t[n].contiguous().to(DEV) for n in ("qT", "kT", "doT")]
        assert all(tuple(x.shape) == (B, H, 64, R) for x in tr)
    g = [torch.full((rows + 8, D), SENT, dtype=torch.bfloat16, device=DEV) for _ in range(3)]
    vl = torch.tensor(lay.lens, dtype=torch.int32, device=DEV)
    fn = lib().sc_attn_bwd_fused_bf16 if entry == "fused" else lib().sc_attn_bwd_bf16
    check(fn(p(d["q"]), D, p(d["k"]), D, p(d["v"]), D, p(d["out"]), D, p(d["dout"]), D, p(tr[0]), p(tr[1]), p(tr[2]), p(d["lse2"]), p(delta),
             p(vl), p(g[0]), D, p(g[1]), D, p(g[2]), D, B, R, H, lay.q_rows, SCALE, int(inst == "causal"), DROP_P if inst == "drop" else 0.0,
             DROP_SEED, ops._stream()), f"sc_attn_bwd ({entry})")
    torch.cuda.synchronize()
    g = [x.cpu() for x in g]
    assert all(bool((x[rows:] == SENT).all()) for x in g), "sentinel rows behind dq / dk / dv were written"
    return {n: x[:rows] for n, x in zip(("dq", "dk", "dv"), g)}


def _base(lay, c, unfused):
    t = {n: c[n] for n in ("q", "k", "v", "dout", "out", "lse2")}
    if unfused:
        t.update(qT=pc.head_transpose(c["q"], lay), kT=pc.head_transpose(c["k"], lay), doT=pc.head_transpose(c["dout"], lay))
    return t


def _poison_keys(lay, c, t, unfused):
    """k^T: finite in the last partly valid 32-key block (0 x k^T), any bits behind it.  Unfused, k^T is the caller's: k itself holds any
    bits on every key t >= len.  Fused, the call transposes k into k^T: k inherits "finite" in that block.  v: N(0, 64^2) where a partly
    valid 128-key block computes with it (tail32, tail128), any bits in wholly padded blocks."""
    K, D = lay.key, lay.D
    t = dict(t)
    if unfused:
        t["k"] = pc.poison_bf16(t["k"], pc.row_mask(~lay.valid, D), pc.NONFINITE_POISON)
    else:
        k = pc.poison_bf16(t["k"], pc.row_mask(K["tail32"], D), pc.FINITE_POISON)
        t["k"] = pc.poison_bf16(k, pc.row_mask(K["tail128"] | K["padded"], D), pc.NONFINITE_POISON)
    v = pc.put(t["v"], pc.row_mask(K["tail32"] | K["tail128"], D), c["scratch"])
    t["v"] = pc.poison_bf16(v, pc.row_mask(K["padded"], D), pc.NONFINITE_POISON)
    if unfused:
        kT = pc.poison_bf16(t["kT"], pc.col_mask_T(lay, K["tail32"]), pc.FINITE_POISON)
        t["kT"] = pc.poison_bf16(kT, pc.col_mask_T(lay, K["tail128"] | K["padded"]), pc.NONFINITE_POISON)
    return t


def _poison_queries(lay, c, t, unfused):
    """q of every row t >= len: N(0, 64^2), put there BEFORE the forward, so that out and lse2 stay the forward's own; out of those rows
    afterwards: finite poison (delta = sum 0 x out).  Unfused: q^T finite poison on the columns the dk/dv kernel multiplies by dS = 0,
    any bits on the columns it never multiplies; dout^T any bits on those."""
    Q, D = lay.query, lay.D
    t = dict(t)
    t["q"], t["lse2"] = c["q1"], c["lse2_1"]
    t["out"] = pc.poison_bf16(c["out1"], pc.row_mask(~lay.valid, D), pc.FINITE_POISON)
    if unfused:
        qT = pc.poison_bf16(pc.head_transpose(c["q1"], lay), pc.col_mask_T(lay, Q["q_pad"] | Q["q_blk"]), pc.FINITE_POISON)
        t["qT"] = pc.poison_bf16(qT, pc.col_mask_T(lay, Q["q_far"]), pc.NONFINITE_POISON)
        t["doT"] = pc.poison_bf16(t["doT"], pc.col_mask_T(lay, Q["q_far"]), pc.NONFINITE_POISON)
    return t


def _poison_far_rows(lay, c, t, unfused):
    """rows behind the last 32-row block the dk/dv kernel visits: q, out, dout, lse2 (and the transposes' columns) hold any bits - no
    gradient of another row depends on them (their own dq does: it is not asserted in this run)"""
    m, D = lay.query["q_far"], lay.D
    t = dict(t)
    for n in ("q", "out", "dout"):
        t[n] = pc.poison_bf16(t[n], pc.row_mask(m, D), pc.NONFINITE_POISON)
    t["lse2"] = pc.poison_f32(t["lse2"], pc.stat_mask(lay, m), pc.NONFINITE_POISON)
    if unfused:
        for n in ("qT", "doT"):
            t[n] = pc.poison_bf16(t[n], pc.col_mask_T(lay, m), pc.NONFINITE_POISON)
    return t


def _against_fp64(rep, tag, lay, inst, c, got):
    """the clean run against attn_cases.bwd_ref fed the forward's own error bounds, as tests/test_gpu_attn_scores.py::_backward"""
    R, H = lay.R, lay.H
    for b, nv in enumerate(lay.lens):
        sl = slice(b * R, (b + 1) * R)
        qh, kh, vh, dh = (_heads(c[n][sl], H) for n in ("q", "k", "v", "dout"))
        mask = ac.key_mask(R, nv, int(inst == "causal"))[None].expand(H, -1, -1)
        mult = ac.drop_mult(ac.drop_index_uniform(b, R, nh=H), DROP_SEED, DROP_P)[0] if inst == "drop" else None
        f = ac.fwd_ref(qh, kh, vh, mask, mult=mult)
        ep, dd = ac.flash_bwd_errors(f, dh)
        r = ac.bwd_ref(qh, kh, vh, dh, f["mask"], mult=mult, ep=ep, ddelta=dd)
        for n in ("dq", "dk", "dv"):
            ac.check(rep, f"{tag} b={b}", n, _heads(got[n][sl], H), r[n], r["bound_" + n])


def _compare(rep, tag, what, lay, got, clean, zero_q):
    valid = lay.valid
    for n in ("dq", "dk", "dv"):
        nbad = int((got[n][valid].view(torch.int16) != clean[n][valid].view(torch.int16)).sum())
        print(f"POISON|{tag}|{what}|{n} of the rows t < len: {nbad} elements differ, {int(torch.isnan(got[n][valid].float()).sum())} NaN")
        rep.require(tag, f"{what}: {n} of the rows t < len differs from the clean run in {nbad} elements", pc.bits_equal(got[n][valid], clean[n][valid]))
    for n in ("dk", "dv"):
        nz = int((got[n][~valid] != 0).sum())
        rep.require(tag, f"{what}: {n} of the keys t >= len is not exactly zero in {nz} elements", nz == 0)
    nz = int((got["dq"][zero_q] != 0).sum())
    rep.require(tag, f"{what}: dq of rows with dout = 0 is not exactly zero in {nz} elements", nz == 0)


@pytest.mark.parametrize("entry", pc.BWD_ENTRIES)
@pytest.mark.parametrize("inst", pc.BWD_INSTANCES)
@pytest.mark.parametrize("name", list(pc.BWD_GEOMETRIES))
def test_attention_backward_ignores_what_it_reads_but_excludes(name, inst, entry):
    lay, c = _case(name, inst)
    unfused = entry == "unfused"
    tag = f"attn_bwd {name} {inst} {entry}"
    rep = ac.Report()
    valid = lay.valid
    # a pad query's own forward values do not reach the valid rows of the forward either
    assert pc.bits_equal(c["out1"][valid], c["out"][valid])
    assert pc.bits_equal(c["lse2_1"][pc.stat_mask(lay, valid)], c["lse2"][pc.stat_mask(lay, valid)])
    assert bool(torch.isfinite(c["out1"].float()).all()) and bool(torch.isfinite(c["lse2_1"]).all())
    base = _base(lay, c, unfused)
    clean = _backward(entry, lay, inst, base, dirty=False)
    assert all(bool(torch.isfinite(x.float()).all()) for x in clean.values())
    assert all(float(clean[n][valid].float().abs().max()) > 0 for n in clean)
    _against_fp64(rep, tag, lay, inst, c, clean)
    _compare(rep, tag, "clean", lay, clean, clean, ~valid)
    keys, queries = _poison_keys(lay, c, base, unfused), _poison_queries(lay, c, base, unfused)
    runs = [("keys t >= len", keys, ~valid), ("query rows t >= len", queries, ~valid),
            ("keys and query rows", _poison_queries(lay, c, keys, unfused), ~valid)]
    if bool(lay.query["q_far"].any()):
        runs.append(("rows behind the last visited query block: any bits", _poison_far_rows(lay, c, keys, unfused), ~valid & ~lay.query["q_far"]))
    for what, t, zero_q in runs:
        _compare(rep, tag, what, lay, _backward(entry, lay, inst, t, dirty=True), clean, zero_q)
    rep.done()


# ================================================================================================================== (b) as weak as stated
def _violations(lay, c):
    """name -> (entry, operands, the outputs that must then differ on their valid rows, whether dk of the keys t >= len must stop being
    zero): ONE region of the clean operands holds more than its class allows"""
    K, Q, D = lay.key, lay.query, lay.D
    fused, unfused = _base(lay, c, False), _base(lay, c, True)
    padq = Q["q_pad"] | Q["q_blk"]
    q_first = _poison_queries(lay, c, fused, False)             # q ~ N(0, 64^2) and the forward's own lse2 on the pad queries
    out = {}
    out["v, last partly valid 32-key block: non-finite"] = ("fused", dict(fused, v=pc.poison_bf16(c["v"], pc.row_mask(K["tail32"], D), pc.NONFINITE_POISON)), ("dq",), True)
    out["k^T, last partly valid 32-key block: non-finite"] = ("unfused", dict(unfused, kT=pc.poison_bf16(unfused["kT"], pc.col_mask_T(lay, K["tail32"]), pc.NONFINITE_POISON)), ("dq",), False)
    out["k, last partly valid 32-key block, fused entry (k^T is made from it): non-finite"] = ("fused", dict(fused, k=pc.poison_bf16(c["k"], pc.row_mask(K["tail32"], D), pc.NONFINITE_POISON)), ("dq",), False)
    out["v, later 32-key blocks of a partly valid 128-key block: non-finite"] = ("fused", dict(fused, v=pc.poison_bf16(c["v"], pc.row_mask(K["tail128"], D), pc.NONFINITE_POISON)), (), True)
    out["q of pad queries: non-finite"] = ("fused", dict(fused, q=pc.poison_bf16(c["q"], pc.row_mask(padq, D), pc.NONFINITE_POISON)), ("dk", "dv"), False)
    out["out of pad queries: non-finite"] = ("fused", dict(fused, out=pc.poison_bf16(c["out"], pc.row_mask(padq, D), pc.NONFINITE_POISON)), ("dk",), False)
    out["lse2 of pad queries: finite, not the forward's"] = ("fused", dict(q_first, lse2=pc.poison_f32(c["lse2_1"], pc.stat_mask(lay, padq), pc.FINITE_POISON)), ("dv",), False)
    return out


def test_attention_backward_contract_is_as_weak_as_stated():
    """Each class of the table is the weakest that holds: one step beyond it and a valid gradient (or a promised zero) changes.  Values
    inside allocated tensors only."""
    name, inst = "R=256", "plain"
    lay, c = _case(name, inst)
    valid = lay.valid
    clean = {e: _backward(e, lay, inst, _base(lay, c, e == "unfused"), dirty=False) for e in pc.BWD_ENTRIES}
    bad = []
    for what, (entry, t, differ, dk_pad) in _violations(lay, c).items():
        got = _backward(entry, lay, inst, t, dirty=False)
        same = {n: pc.bits_equal(got[n][valid], clean[entry][n][valid]) for n in ("dq", "dk", "dv")}
        pad_nz = int((got["dk"][~valid] != 0).sum())
        print(f"POISON|attn_bwd {name} {inst} {entry}|beyond the class: {what}|valid rows bit-equal {same}|dk of keys t >= len: {pad_nz} elements not zero")
        if any(same[n] for n in differ) or (dk_pad and pad_nz == 0):
            bad.append(what)
        if not differ and not all(same.values()):                # tail128: the valid rows must NOT notice
            bad.append(what + " (valid rows changed)")
    assert not bad, bad


# ================================================================================================================== (c) attn32, row reducers
def test_short_attention_backward_ignores_rows_behind_a_prompt():
    """sc_attn32_bwd_bf16, 3 sequences with prompts of 32 / 1 / 17 rows, dout zero behind each: qkv behind a prompt holds zeros or
    N(0, 64^2) -> dqkv of the prompt rows keeps its bits, dqkv behind a prompt is exactly zero"""
    ops = _ops()
    H, W = 2, 128
    valid = pc.short_valid()
    M = valid.numel()
    g = torch.Generator().manual_seed(77)
    qkv = torch.zeros(M, 3 * W)
    qkv[valid] = torch.randn(int(valid.sum()), 3 * W, generator=g)
    dout = torch.zeros(M, W)
    dout[valid] = torch.randn(int(valid.sum()), W, generator=g)
    junk = pc.ORDINARY * torch.randn(M, 3 * W, generator=g)
    qkv, dout, junk = qkv.to(torch.bfloat16), dout.to(torch.bfloat16), junk.to(torch.bfloat16)
    clean = ops.attn32_bwd(qkv.to(DEV), dout.to(DEV), H, SCALE).cpu()
    with pc.poisoned_empty():
        got = ops.attn32_bwd(pc.put(qkv, pc.row_mask(~valid, 3 * W), junk).to(DEV), dout.to(DEV), H, SCALE).cpu()
    nbad = int((got[valid].view(torch.int16) != clean[valid].view(torch.int16)).sum())
    print(f"POISON|attn32_bwd prompts {pc.SHORT_PROMPTS}|rows behind a prompt ~ N(0, 64^2)|prompt rows: {nbad} elements differ|"
          f"behind: {int((got[~valid] != 0).sum())} not zero")
    assert bool(torch.isfinite(clean.float()).all()) and float(clean[valid].float().abs().max()) > 0
    assert pc.bits_equal(got[valid], clean[valid])
    assert bool((clean[~valid] == 0).all()) and bool((got[~valid] == 0).all())


def _reducer(kind, dirty):
    """one row-reducing gradient kernel at rows = 3 x 128, valid rows 128 / 1 / 37, dy exactly zero on the pad rows -> (outputs, dx or
    None).  ``dirty``: the other operand's pad rows hold the strongest poison its class allows and torch.empty returns NaN."""
    ops = _ops()
    valid = pc.reducer_valid()
    rows, nv = valid.numel(), int(valid.sum())
    g = torch.Generator().manual_seed(500 + pc.REDUCERS.index(kind))
    bf = lambda x: x.to(torch.bfloat16)

    def on_valid(cols, scale=1.0, shift=0.0):
        t = torch.zeros(rows, cols)
        t[valid] = torch.randn(nv, cols, generator=g) * scale + shift
        return bf(t)

    def finite(t):
        return pc.poison_bf16(t, pc.row_mask(~valid, t.shape[1]), pc.FINITE_POISON) if dirty else t

    def ordinary(t):
        junk = bf(pc.ORDINARY * torch.randn(t.shape, generator=g))
        return pc.put(t, pc.row_mask(~valid, t.shape[1]), junk) if dirty else t

    f32 = lambda *s: torch.randn(*s, generator=g).to(DEV)
    dx = None
    if kind in ("wgrad_tn", "wgrad_transposing"):
        N, K = (256, 256) if kind == "wgrad_tn" else (48, 96)
        dy, x, gW, gb = on_valid(N), finite(on_valid(K)), f32(N, K), f32(N)
        ops.wgrad_bf16(dy.to(DEV), x.to(DEV), gW, gb)
        outs = [gW, gb]
    elif kind == "wgrad_list":
        N, K = 768, 256
        dy, x = on_valid(N), finite(on_valid(K))
        outs = [f32(256, K) for _ in range(3)]
        ops.wgrad_bf16(dy.to(DEV), x.to(DEV), outs, None, beta=1.0)
    elif kind == "colsum":
        # no second operand: x is a column slice of a wider buffer whose other columns hold NaN / Inf on every row
        wide = torch.zeros(rows, 320, dtype=torch.bfloat16)
        wide[:, 32: 288] = on_valid(256)
        if dirty:
            m = torch.ones(rows, 320, dtype=torch.bool)
            m[:, 32: 288] = False
            wide = pc.poison_bf16(wide, m, pc.NONFINITE_POISON)
        out = f32(256)
        ops.colsum_bf16(wide.to(DEV)[:, 32: 288], out, beta=1.0)
        outs = [out]
    elif kind in ("ln_acc", "ln_acc_drop_sum", "ln_dres"):
        D = 256
        dy, x = on_valid(D), ordinary(on_valid(D, 1.5, 0.3))           # x enters the row's mean and variance: ordinary magnitude
        dres = on_valid(D) if kind == "ln_dres" else None
        gamma, acc = 1.0 + 0.1 * f32(D), (f32(D), f32(D))
        kw = {"dres": dres.to(DEV)} if dres is not None else {}
        if kind == "ln_acc_drop_sum":
            s = f32(D)
            dx, dxd = ops.layernorm_bwd(x.to(DEV), dy.to(DEV), gamma, 1e-5, acc=acc, drop=(0.1, 777), sum_acc=s)
            outs = [dx, dxd, acc[0], acc[1], s]
        else:
            dx = ops.layernorm_bwd(x.to(DEV), dy.to(DEV), gamma, 1e-5, acc=acc, **kw)
            outs = [dx, acc[0], acc[1]]
    elif kind == "posconv_wgrad":
        # slabs [G, B, Rp, Dg], frames at rows halo .. halo + R.  xg is the convolution's zero padding wherever a window of a valid frame
        # reaches (rows < halo + len + Kp - 1 of an utterance): exact zeros there are mathematics, not scratch.  The rows behind meet
        # du = 0 only: finite poison.
        Dg, G, B, R, Kp, halo = 48, 2, 3, 128, 128, 64
        Rp = R + 2 * halo
        v3 = valid.view(B, R)
        xg = torch.zeros(G, B, Rp, Dg)
        xg[:, :, halo: halo + R][:, v3] = torch.randn(G, nv, Dg, generator=g)
        du_buf = torch.zeros((G * B * Rp + halo + 1) * Dg)
        du_buf[: G * B * Rp * Dg].view(G, B, Rp, Dg)[:, :, halo: halo + R][:, v3] = torch.randn(G, nv, Dg, generator=g)
        xg = bf(xg)
        if dirty:
            m = torch.zeros(G, B, Rp, Dg, dtype=torch.bool)
            for b, n in enumerate(pc.REDUCER_LENS):
                m[:, b, n + Kp:] = True                      # du row t (slab row t of the advanced view) reads xg rows t .. t + Kp - 1
            assert int(m.sum()) > 0
            xg = pc.poison_bf16(xg, m, pc.FINITE_POISON)
        outs = [ops.posconv_wgrad(bf(du_buf).to(DEV)[halo * Dg:], xg.to(DEV), G, B * Rp, Dg, Kp)]
    elif kind == "wsum_seg":
        # h [NL, rows, D] in the segment layout (pitch 128: pad rows INSIDE a pitch), g [B, R, D] uniform with the frames at row offset 1.
        # The kernel forms g . (h_n - h_last): h of the pad rows is of ordinary magnitude, g of the rows it skips holds any bits.
        NL, D, B, R = 13, 256, 3, 136
        seg = ops.RowSegments([pc.REDUCER_PITCH] * B, pc.REDUCER_LENS, DEV)
        h = torch.stack([ordinary(on_valid(D)) for _ in range(NL)])
        gr = torch.zeros(B, R, D)
        gr[:, 1: 1 + pc.REDUCER_PITCH][valid.view(B, -1)] = torch.randn(nv, D, generator=g)
        if dirty:
            m = torch.zeros(B, R, D, dtype=torch.bool)
            m[:, 0] = True
            m[:, 1 + pc.REDUCER_PITCH:] = True
            gr = pc.poison_f32(gr, m, pc.NONFINITE_POISON)
        w = torch.softmax(torch.randn(NL, generator=g), 0).to(DEV)
        outs = [ops.wsum_bwd_logits(h.to(DEV), gr.to(DEV), w, B, R, D, 1, seg=seg)]
    else:
        raise KeyError(kind)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs], (None if dx is None else dx.cpu())


@pytest.mark.parametrize("kind", pc.REDUCERS)
def test_row_reducers_ignore_pad_rows_under_a_zero_gradient(kind):
    valid = pc.reducer_valid()
    clean, dx = _reducer(kind, False)
    with pc.poisoned_empty():
        got, dx_p = _reducer(kind, True)
    same = [pc.bits_equal(a, b) for a, b in zip(got, clean)]
    print(f"POISON|{kind} rows 3 x 128 valid {pc.REDUCER_LENS}|pad rows poisoned, torch.empty = NaN|outputs bit-equal {same}|"
          f"NaN {[int(torch.isnan(a.float()).sum()) for a in got]}")
    assert all(bool(torch.isfinite(a.float()).all()) for a in clean) and all(float(a.float().abs().max()) > 0 for a in clean)
    assert all(same), (kind, same)
    if dx is not None:
        assert bool((dx[~valid] == 0).all()) and bool((dx_p[~valid] == 0).all()), "dx of a pad row is not exactly zero"


# ================================================================================================================== (d) whole train steps
# 3-layer base with unfreeze_layers = [1, 2] (also with the encoder's dropout on), 2-layer fully trainable base and large, 2-layer frozen base
MODELS = ("base3-unfreeze12", "base3-unfreeze12-dropout", "base2-trainable", "large2-trainable", "base2-frozen-ragged", "base2-frozen-padded")
SHORT = 320                     # samples: one valid frame (ceil(320 / (L // T)) = 1) and feat_len = round(320 / 320) = 1


def _build(kind):
    from speechclip_plus_amd import (KWClip_GeneralTransformer, base_parallel_config, large_parallel_config, random_hubert_state_dict,
                                     set_dropout)
    from speechclip_plus_amd.speech_encoder import ARCHS
    large = kind.startswith("large")
    layers = 3 if kind.startswith("base3") else 2
    arch = dataclasses.replace(ARCHS["hubert_large_ll60k" if large else "hubert"], layers=layers, feature_grad_mult=0.1)
    sd = random_hubert_state_dict(arch, seed=29)
    torch.manual_seed(29)
    cfg = large_parallel_config() if large else base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    if "frozen" not in kind:
        cfg.audio_encoder.trainable = True
        if "unfreeze" in kind:
            cfg.audio_encoder.unfreeze_layers = [1, 2]
    model = set_dropout(KWClip_GeneralTransformer(cfg, device="cuda:0", hubert_state_dict=sd, hubert_arch=arch).train(), False)
    enc = model.audio_encoder
    with torch.no_grad():
        enc.weightedsum_layer.weights.copy_(torch.tensor([0.2, -0.1, 0.4, 0.3][: layers + 1]))
    if "dropout" in kind:
        enc.hubert_dropout = True           # fairseq's train-mode dropout in the frozen and the unfrozen layers (hash masks)
    if "frozen" in kind:
        enc.ragged = "ragged" in kind
    return model


def _batch(kind, lens, seed):
    g = torch.Generator().manual_seed(seed)
    B, E = len(lens), 768 if kind.startswith("large") else 512
    wav = torch.zeros(B, max(lens))
    for b, l in enumerate(lens):
        wav[b, :l] = torch.randn(l, generator=g) * 0.5
    ids = torch.tensor([0, 1, 1, 2, 3][:B])
    return {"wav": wav.cuda(), "wav_len": torch.tensor(lens), "image": torch.randn(B, E, generator=g).cuda(), "id": ids.cuda()}


def _step(model, batch):
    """model(batch), compute_loss, backward -> {"loss": ..., parameter name: grad} on the CPU"""
    enc = model.audio_encoder
    model.zero_grad(set_to_none=True)
    torch.manual_seed(31)                   # the dropout seeds are a function of torch's seed and of the forward count
    enc._drop_calls = 0
    loss = model.compute_loss(model(batch)[0])["loss"]
    loss.backward()
    torch.cuda.synchronize()
    res = {"loss": loss.detach().float().cpu().reshape(1)}
    res.update({n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None})
    model.zero_grad(set_to_none=True)
    return res


def _same_step(tag, what, got, clean):
    assert set(got) == set(clean), set(got) ^ set(clean)
    diff = [n for n in clean if not pc.bits_equal(got[n], clean[n])]
    nan = {n: int(torch.isnan(got[n].float()).sum()) for n in got}
    print(f"POISON|train step {tag}|{what}|{len(clean)} results, {len(diff)} differ|NaN {sum(nan.values())} of {sum(t.numel() for t in got.values())}")
    for n in clean:
        if nan[n] or n in diff:
            print(f"POISON|train step {tag}|{what}|{n}|NaN {nan[n]} of {got[n].numel()}|bits equal {n not in diff}")
    return diff


@pytest.mark.parametrize("kind", MODELS)
def test_train_step_does_not_depend_on_unwritten_memory_or_history(kind):
    frozen = "frozen" in kind
    # the lengths of tests/test_gpu_model.py plus one utterance of a single valid frame; A: other lengths in the same plan (the uniform
    # layout of a trainable encoder has one plan per padded length, the segment layout one per 2 s bucket: A is longer there)
    lens_b = [9000, 6100, SHORT, 4100, 8000] if kind.startswith("base3") else [9000, 6100, SHORT, 4100]
    lens_a = [20000, 12000, 15000, 7000] if frozen else [5000, 9000, 7777, 2000, 640][: len(lens_b)]
    model = _build(kind)
    enc = model.audio_encoder
    B, A = _batch(kind, lens_b, 41), _batch(kind, lens_a, 42)
    last_plan = lambda: next(reversed(enc._plans.values()))      # the plan of the forward that ran last (speech_encoder._plan)
    clean = _step(model, B)
    assert last_plan().seg_mode == frozen, "trainable encoders run the uniform row layout (speech_encoder._seg_mode): enc.ragged is not consulted"
    assert all(bool(torch.isfinite(t.float()).all()) for t in clean.values())
    if not frozen:                          # every encoder parameter that trains is among the compared gradients
        named = {id(p): n for n, p in model.named_parameters()}
        enc_names = [named[id(p)] for p in enc.train_layers.parameters()]
        assert sum(n in clean and float(clean[n].float().abs().max()) > 0 for n in enc_names) >= 15 * len(enc.train_layers.ids), enc_names
    bad = {}
    bad["a second clean step"] = _same_step(kind, "a second clean step", _step(model, B), clean)
    with pc.poisoned_empty():
        warm = _step(model, B)
    bad["torch.empty = NaN, warm model"] = _same_step(kind, "torch.empty = NaN, warm model", warm, clean)
    # history: A, then B twice - a frozen encoder that runs ahead on its own stream alternates between two plans, so the SECOND of the
    # two B steps is the one that finds A's leftovers there; without that schedule the first one does
    other = _step(model, A)
    plan_a = last_plan()
    assert all(bool(torch.isfinite(t.float()).all()) for t in other.values())
    plans_b = []
    for what in ("the step after a step on another batch", "the second step after a step on another batch"):
        again = _step(model, B)
        plans_b.append(last_plan())
        bad[what] = _same_step(kind, what, again, clean)
    assert any(p is plan_a for p in plans_b), "batch A was meant to run in a plan that batch B then runs in"
    if not frozen:                          # the other setting of enc.ragged: same layout, same bits
        enc.ragged = not enc.ragged
        bad["enc.ragged flipped"] = _same_step(kind, "enc.ragged flipped", _step(model, B), clean)
    del model
    fresh = _build(kind)
    with pc.poisoned_empty():
        first = _step(fresh, B)
    bad["torch.empty = NaN, first step of a fresh model"] = _same_step(kind, "torch.empty = NaN, first step of a fresh model", first, clean)
    assert not any(bad.values()), {k: v for k, v in bad.items() if v}
