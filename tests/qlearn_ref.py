"""numpy restatement of the Q-learning guided sampler, written from the definition in the header comment of csrc/rt_qlearn.h (grid cells
over a box, 64 equal-area patches = 8 bands in z x 8 sectors in phi, P = (1 - eps) Q / sum Q + eps / 64, 48.16 fixed-point rewards,
Q <- (1 - alpha) Q + alpha mean, V = Q times the clamped cosines of the patch centres) -- not from either C++ statement of it.  float32
step by step, sums left to right, no fused multiply-add; transcendentals are float64 rounded once (DESIGN "Transcendentals").  Whole arrays
at a time: a pick is a count of the cumulative sums a draw has passed, not a loop with a break.  No device and no product code; the random
streams are tests/filter_ref.py's.  tests/test_qlearn_cpu.py holds the oracle (oracle/orc_qlearn.h) to this, tests/test_gpu_qlearn.py the
device."""
import numpy as np

from filter_ref import random_float, stream_seed  # noqa: F401  (stream_seed: re-exported for the callers)

f32 = np.float32
PATCHES, BANDS, SECTORS = 64, 8, 8
Q_MIN = f32(1e-4)
REWARD_MAX = f32(64.0)
SECTOR_ANGLE = f32(f32(6.28318530717958647692528) * f32(0.125))


def _f(a):
    return np.asarray(a, dtype=np.float32)


def inv_of(grid, lo, hi):
    """cells per unit length on each axis"""
    return f32(grid) / (_f(hi) - _f(lo))


def cell(grid, lo, hi, x):
    """the cell of each point of x [n, 3]: floor((x - lo) * grid / (hi - lo)) per axis, held inside 0 .. grid - 1 (a NaN coordinate: 0),
    x fastest"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = (_f(x).reshape(-1, 3) - _f(lo)) * inv_of(grid, lo, hi)
        k = np.where(f > 0, np.floor(np.minimum(f, f32(grid))), f32(0))  # (NaN > 0 is false)
    k = np.minimum(k.astype(np.int64), grid - 1)
    return ((k[:, 2] * grid + k[:, 1]) * grid + k[:, 0]).astype(np.int64)


def patch_of(n):
    """the patch a vector points into: band = floor((z + 1) * 4) held inside 0 .. 7; the sector from the quadrant of (x, y) -- the
    half-plane y >= 0 (so y = -0.0) is the upper one, x = 0 belongs to the quadrant on its left there and on its right below -- and
    which of |x|, |y| is larger, a tie going to the later sector; (0, 0, z) is sector 0"""
    n = _f(n).reshape(-1, 3)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(invalid="ignore"):
        fz = (z + f32(1)) * f32(4)
        band = np.where(fz > 0, np.floor(np.minimum(fz, f32(7))), f32(0)).astype(np.int64)
        ax, ay = np.abs(x), np.abs(y)
        upper = y >= 0
        quadrant = np.where(upper, np.where(x > 0, 0, 1), np.where(x < 0, 2, 3))
        # even quadrants start at the x axis, odd ones at the y axis
        second = np.where(quadrant % 2 == 0, ~(ay < ax), ~(ax < ay))
        sector = 2 * quadrant + second.astype(np.int64)
        sector = np.where((x == 0) & (y == 0), 0, sector)
    return 8 * band + sector


def direction(i, j, u1, u2):
    """the direction of band i, sector j at (u1, u2): z = -1 + (i + u1) / 4, phi = (j + u2) * pi / 4"""
    i, j, u1, u2 = np.broadcast_arrays(np.asarray(i), np.asarray(j), _f(u1), _f(u2))
    z = f32(-1) + (i.astype(np.float32) + u1) * f32(0.25)
    phi = (j.astype(np.float32) + u2) * SECTOR_ANGLE
    s = np.sqrt(np.maximum(f32(0), f32(1) - z * z)).astype(np.float32)
    c = np.cos(phi.astype(np.float64)).astype(np.float32)
    sn = np.sin(phi.astype(np.float64)).astype(np.float32)
    return np.stack([s * c, s * sn, z], axis=-1).astype(np.float32)


def centres():
    """[64, 3]: every patch at (1/2, 1/2)"""
    p = np.arange(PATCHES)
    return direction(p // 8, p % 8, f32(0.5), f32(0.5))


def weights():
    """[64, 64]: max(0, d_m . d_p) of the centres, the dot as (x x + y y) + z z"""
    d = centres()
    a, b = d[:, None, :], d[None, :, :]
    dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    return np.where(dot > 0, dot, f32(0)).astype(np.float32)


_WEIGHTS = None


def band_sums(q):
    """[cells, 8]: each band's eight values added in sector order"""
    q = _f(q).reshape(-1, BANDS, SECTORS)
    b = np.zeros(q.shape[:2], np.float32)
    for j in range(SECTORS):
        b = b + q[:, :, j]
    return b


def derive(q):
    """(band sums [cells, 8], V [cells, 64]): V[cell][m] = sum over p, in patch order, of Q[cell][p] * weights[m][p]"""
    global _WEIGHTS
    if _WEIGHTS is None:
        _WEIGHTS = weights()
    q = _f(q).reshape(-1, PATCHES)
    v = np.zeros((len(q), PATCHES), np.float32)
    for p in range(PATCHES):
        v = v + q[:, p, None] * _WEIGHTS[None, :, p]
    return band_sums(q), v


def apply(q, sums, counts, alpha):
    """the fold between batches: (the new Q, the sums and the counts it leaves).  Where a count is not 0: mean = sum / (count * 65536)
    in float64, rounded once; Q <- (1 - alpha) Q + alpha mean, not below Q_MIN; the entry's sum and count return to 0."""
    q, alpha = _f(q), f32(alpha)
    sums, counts = np.asarray(sums, np.int64), np.asarray(counts, np.uint32)
    paid = counts != 0
    mean = (sums.astype(np.float64) / (np.where(paid, counts, 1).astype(np.float64) * 65536.0)).astype(np.float32)
    new = (f32(1) - alpha) * q + alpha * mean
    with np.errstate(invalid="ignore"):
        new = np.where(new > Q_MIN, new, Q_MIN)
    return np.where(paid, new, q).astype(np.float32), np.where(paid, 0, sums).astype(np.int64), np.where(paid, 0, counts).astype(np.uint32)


def reward_fixed(R):
    """a reward as the integer that is added: held inside [0, 64] (a NaN: 0), times 65536, rounded to the nearest integer, ties to even"""
    R = _f(R)
    with np.errstate(invalid="ignore"):
        R = np.where(R >= 0, np.where(R < REWARD_MAX, R, REWARD_MAX), f32(0)).astype(np.float32)
    return np.rint((R * f32(65536.0)).astype(np.float64)).astype(np.int64)


def lum(c):
    c = _f(c)
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def sample(rows, eps, state):
    """one guided pick per (row of 64 values, stream state): four draws -- mixture, patch, two inside the patch.
    Returns dict(patch, P, dir, state (after the draws), u (the four draws), branch: 'eps' | 'cdf' per pick, last_band / last_sector: no
    earlier band / sector took the draw, past_end: the draw is not below the last cumulative sum either)."""
    rows, eps = _f(rows).reshape(-1, PATCHES), f32(eps)
    n = len(rows)
    b = band_sums(rows)
    T = np.zeros(n, np.float32)
    for i in range(BANDS):
        T = T + b[:, i]
    s = np.asarray(state, np.uint32)
    s, u_sel = random_float(s)
    s, u_pick = random_float(s)
    s, u1 = random_float(s)
    s, u2 = random_float(s)
    uniform = (u_sel < eps) | ~(T > 0)
    # the uniform pick
    p_uni = np.minimum((u_pick * f32(64)).astype(np.int64), 63)
    # the pick by the table: the bands whose cumulative sum the draw has passed, then the same inside the band
    x = u_pick * T
    cum = np.zeros((n, BANDS), np.float32)
    acc = np.zeros(n, np.float32)
    for i in range(BANDS):
        acc = acc + b[:, i]
        cum[:, i] = acc
    band = np.cumprod(~(x[:, None] < cum[:, :7]), axis=1).sum(1)   # (a count of leading 'passed': cum never falls for positive values)
    before = np.where(band > 0, cum[np.arange(n), np.maximum(band - 1, 0)], f32(0))
    x2 = x - before
    vals = rows.reshape(n, BANDS, SECTORS)[np.arange(n), band]
    cum2 = np.zeros((n, SECTORS), np.float32)
    acc = np.zeros(n, np.float32)
    for j in range(SECTORS):
        acc = acc + vals[:, j]
        cum2[:, j] = acc
    sector = np.cumprod(~(x2[:, None] < cum2[:, :7]), axis=1).sum(1)
    p_cdf = 8 * band + sector
    patch = np.where(uniform, p_uni, p_cdf)
    qp = rows[np.arange(n), patch]
    with np.errstate(invalid="ignore", divide="ignore"):
        P = np.where(T > 0, (f32(1) - eps) * (qp / T) + eps * f32(1.0 / 64), f32(1.0 / 64)).astype(np.float32)
    return dict(patch=patch, P=P, dir=direction(patch // 8, patch % 8, u1, u2), state=s, u=(u_sel, u_pick, u1, u2),
                branch=np.where(uniform, "eps", "cdf"),
                last_band=~uniform & (band == 7), last_sector=~uniform & (sector == 7),
                past_end=~uniform & (~(x < cum[:, 7]) | ~(x2 < cum2[:, 7])))


class Table:
    """what rt_qlearn_enable sets up: a table at q_init, empty sums"""

    def __init__(self, grid, lo, hi, alpha=0.3, eps=0.2, q_init=1.0, learn_mask=0):
        self.grid, self.lo, self.hi, self.alpha, self.eps, self.learn_mask = grid, _f(lo), _f(hi), f32(alpha), f32(eps), int(learn_mask)
        self.cells = grid ** 3
        self.q = np.full((self.cells, PATCHES), f32(q_init), np.float32)
        self.sums, self.counts = np.zeros((self.cells, PATCHES), np.int64), np.zeros((self.cells, PATCHES), np.uint32)

    def cell(self, x):
        return cell(self.grid, self.lo, self.hi, x)

    def apply(self):
        self.q, self.sums, self.counts = apply(self.q, self.sums, self.counts, self.alpha)

    def learner(self, state):
        return (np.asarray(state, np.uint32) & np.uint32(self.learn_mask)) == 0

    def sample(self, cells, state):
        return sample(self.q[np.asarray(cells)], self.eps, state)
