"""The quantiser's soft / Gumbel / learnable-temperature modes restated on the host (csrc/vq.hip under
vector_quantizers.SimpleVectorQuantizer), written from the formulas of include/speechclip_hip.h - no autograd, no reference code:

  * the numpy uint32 twin of the stateless noise: e = n V + v, w = hash32(e ^ seed), u = ((w >> 9) + 0.5) 2^-23, g = -log(-log u);
  * an fp64 reference of every mode's ``subword_prob``, targets, keywords and of the gradients
        dz = s (t - <s, t>),   dx = dz / tau,   d tau = -(1 / tau) sum dz z  (over s > 0),   t = d subword_prob;
  * the error bounds the GPU tests assert, derived from the number formats and the kernels' operation counts (never from what the
    kernels return).

Nothing here needs a GPU; tests/test_vq_modes_cases_cpu.py checks this file against the reference's fixtures and F.gumbel_softmax.
"""
import numpy as np

U = 2.0 ** -24                     # fp32 unit roundoff
G_MIN, G_MAX = -2.82, 16.64        # -log(-log u) over u in [2^-24, 1 - 2^-24]
SPECIAL = (0, 2, 3)


# ---------------------------------------------------------------------------------------------------- the noise
def hash32(x):
    """lowbias32, the kernels' sc_hash32, on a uint32 array (wrap-around arithmetic)."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def noise_words(Nk, V, seed):
    assert Nk * V < 1 << 32
    e = (np.arange(Nk, dtype=np.uint64)[:, None] * np.uint64(V) + np.arange(V, dtype=np.uint64)[None, :]).astype(np.uint32)
    return hash32(e ^ np.uint32(seed & 0xffffffff))


def uniform(words):
    """u = ((w >> 9) + 0.5) 2^-23 in fp64: a 24-bit number, the same value the kernel holds in fp32."""
    return ((words >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(Nk, V, seed):
    """g [Nk, V] fp64 = -log(-log u)."""
    return -np.log(-np.log(uniform(noise_words(Nk, V, seed))))


def noise_bound(g):
    """|g_device - g| <= 4 U (1 + |g|): two logarithms of 1 ulp = 2 U each (the inner one's relative error is an absolute error of
    the outer one)."""
    return 4.0 * U * (1.0 + np.abs(g))


# ---------------------------------------------------------------------------------------------------- the modes in fp64
def masked(x, cols=SPECIAL):
    x = np.array(x, dtype=np.float64)
    x[:, [c for c in cols if c < x.shape[1]]] = -np.inf
    return x


def first_argmax(y):
    return np.argmax(y, axis=-1)             # numpy returns the first of equal maxima: the kernels' tie rule


def softmax_lse(z):
    m = z.max(axis=-1, keepdims=True)
    e = np.exp(z - m)
    st = e.sum(axis=-1, keepdims=True)
    return e / st, (m + np.log(st))[:, 0]


def row_statistics(y, tau):
    """-> (m = max y, ls = log sum exp((y - m) / tau)) per row: the pair the kernels keep apart; LSE(y / tau) = m / tau + ls."""
    m = y.max(axis=-1)
    return m, np.log(np.exp((y - m[:, None]) / tau).sum(axis=-1))


def forward(x, tau, hard, g=None, table=None):
    """x [Nk, V] masked fp64, g the noise or None -> dict(s, lse, targets, prob, keywords): the table of the four training modes."""
    y = x if g is None else x + g
    s, lse = softmax_lse(y / tau)
    idx = first_argmax(y)
    prob = s
    if hard:
        prob = np.zeros_like(s)
        prob[np.arange(len(idx)), idx] = 1.0
    out = dict(s=s, lse=lse, z=y / tau, targets=idx, prob=prob)
    if table is not None:
        out["keywords"] = prob @ np.asarray(table, dtype=np.float64)
    return out


def backward(s, z, t, tau):
    """t = d subword_prob [Nk, V] -> (dz, dx, d tau, m = <s, t>); columns with s == 0 get exactly 0 and never meet t or z."""
    live = s > 0
    ts = np.where(live, t, 0.0)
    m = (s * ts).sum(axis=-1, keepdims=True)
    dz = np.where(live, s * (ts - m), 0.0)
    dtau = -(dz * np.where(live, z, 0.0)).sum() / tau
    return dz, dz / tau, dtau, m


def eval_forward(x):
    """eval mode of every configuration: the hard one-hot of the unperturbed argmax."""
    return forward(x, 1.0, True)


# ---------------------------------------------------------------------------------------------------- bounds
def score_abs_bound(x, noise):
    """dy / U: the absolute error of the device's y = x + g in units of U - 4 (1 + G) for the noise's own error and X + G for the
    rounding of the sum (X = max |x| unmasked, G = 16.64); without noise y = x exactly: 0."""
    X = float(np.abs(x[np.isfinite(x)]).max())
    return (4.0 * (1.0 + G_MAX) + X + G_MAX) if noise else 0.0


def prob_rel_bound(x, tau, noise, V):
    """E_s: relative error of the device's s = exp(fma(y - m, 1 / tau, -ls)) against the fp64 s of the same x (and the twin's g), where
    m = max y and ls = log sum exp((y - m) / tau) are kept apart (|a| <= 104 for the exponent a of a normal s, ls <= log V <= 10):
      d = y - m      2 dy (both carry dy) + U |d|;  |d| / tau = |a + ls| <= 114
      a              2 dy / tau + 2 U 114 (the rounding of d, of 1 / tau) + |d ls| + 104 U (the fma's one rounding)
      ls             2 dy / tau + the terms' own 2 U |a'| + 2 U (expf), weighted by p: <= 2 U (H + ls) + 2 U <= 42 U; the sum over 256 lanes
                     + a 64-lane and a 4-wave tree: ceil(V / 256) + 8 additions; logf: 2 U |ls| <= 20 U
      expf           2 U
    E_s = U [4 dy / (U tau) + ceil(V / 256) + 404].  Without noise dy = 0: E_s does not depend on the temperature."""
    return U * (4.0 * score_abs_bound(x, noise) / tau + np.ceil(V / 256.0) + 404.0)


def rowstats_bounds(x, tau, noise, V):
    """-> (|m_dev - m| <= dy, |ls_dev - ls| <= 2 dy / tau + (ceil(V / 256) + 70) U): see prob_rel_bound."""
    dy = U * score_abs_bound(x, noise)
    return dy + 1e-300, 2.0 * dy / tau + (np.ceil(V / 256.0) + 70.0) * U


def soft_slices(Vp):
    units = 3 * Vp // 64
    return max(s for s in range(1, 17) if units % s == 0)


def keyword_k_eff(V):
    """The soft product's accumulation: the contraction of 3 Vp bf16 products (every product exact in fp32) is cut into S equal
    slices, each accumulated serially in fp32 on the matrix pipe (Kc = 3 Vp / S additions), the S partials added in slice order."""
    Vp = -(-V // 128) * 128
    S = soft_slices(Vp)
    return 3 * Vp // S + S


def keyword_bound(s, table, E_s, V):
    """|kw_device - s64 . table64| <= (3 * 2^-18 + E_s + 2 U (K_eff + 3)) (s . |table|), element-wise: the dropped lo lo term and the
    two second roundings (2^-9 2^-9 each, three of them), the relative error of s, the accumulation."""
    return (3.0 * 2.0 ** -18 + E_s + 2.0 * U * (keyword_k_eff(V) + 3)) * (s @ np.abs(table))


def dx_bound(s, t, tau, E_s, V, bf16=False):
    """dx = s (t - m) / tau, m = <s, t>:  s carries E_s, m carries E_s + (ceil(V / 256) + 9) U on <s, |t|> (fma chain + trees), the
    subtraction, the two products and 1 / tau one U each on |t| + |m|;  bf16 output: 2^-9 of the value on top."""
    at = np.where(s > 0, np.abs(t), 0.0)
    ma = (s * at).sum(axis=-1, keepdims=True)
    b = (2.0 * E_s + (np.ceil(V / 256.0) + 9.0 + 4.0) * U) * s * (at + ma) / tau
    return b * (1.0 + 2.0 ** -9) + (2.0 ** -9 * s * (at + ma) / tau if bf16 else 0.0)


def dtau_bound(x, s, z, t, tau, E_s, V, noise):
    """d tau = -(1 / tau) sum dz z  ->  (bound, charged = sum |dz z| / tau).  The accumulation is charged on sum |dz z| / tau: the
    products, a 256-lane strided fma chain + trees per row (ceil(V / 256) + 8), Nk rows added in index order, 1 / tau: one U each.
    The two factors bring their own errors, which cancellation in t - m keeps from being relative to |dz z|:
      |d dz| <= tau * dx_bound (fp32 output),   |d z| <= U [4 (1 + G) noise + 2 (X + G)] / tau   (see prob_rel_bound)."""
    live = s > 0
    az = np.where(live, np.abs(z), 0.0)
    dz = backward(s, z, t, tau)[0]
    charged = (np.abs(dz) * az).sum() / tau
    X = float(np.abs(x[np.isfinite(x)]).max())
    G = G_MAX if noise else 0.0
    dzabs = U * (score_abs_bound(x, noise) + 2.0 * (X + G)) / tau                    # dy, then 1 / tau and the product rounded
    factors = ((tau * dx_bound(s, t, tau, E_s, V)) * az).sum() / tau + np.abs(dz).sum() * dzabs / tau
    return (np.ceil(V / 256.0) + 8.0 + s.shape[0] + 4.0) * U * charged + factors, charged


# ---------------------------------------------------------------------------------------------------- the two conditions
def sampling_counts(seed, Nk=65536, V=16):
    """argmax(x + g) over Nk rows of x = linspace(-1, 1, V) with the special columns masked -> (counts [V], expected Nk p, sigma)."""
    x = masked(np.tile(np.linspace(-1.0, 1.0, V), (Nk, 1)))
    idx = first_argmax(x + gumbel(Nk, V, seed))
    p = softmax_lse(x[:1])[0][0]
    return np.bincount(idx, minlength=V), Nk * p, np.sqrt(Nk * p * (1.0 - p))


SAMPLING_SEEDS = (1, 12345, 0x9E3779B1, 0xDEADBEEF, 7)


def margin_case():
    """x = 0.1 randn(300, 1000) fp32 (seed 0), noise seed 99 -> (x masked fp64, g, smallest top-2 margin of x + g)."""
    x = masked((0.1 * np.random.default_rng(0).standard_normal((300, 1000))).astype(np.float32))
    g = gumbel(300, 1000, 99)
    top = np.sort(x + g, axis=-1)[:, -2:]
    return x, g, float((top[:, 1] - top[:, 0]).min())
