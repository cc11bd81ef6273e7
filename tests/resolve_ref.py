"""numpy restatement of rt_resolve (k_resolve) and the value sets that probe it.  A plain helper module of the test suite:
tests/test_oracle_cpu.py holds it against the oracle's Renderer::ResolvePixel, tests/test_gpu_output_stages.py holds the kernel against it.

RGBF32_to_RGB8(accumulator / it), step by step as oracle/orc_render.h ResolvePixel writes it:
  v = acc / it in f32; m = v if v < 1 else 1 (NaN gives 1); s = f32(255 m);
  q = trunc(s) as int64 where -9.2e18 < s < 9.2e18 (f32 bounds), INT64_MIN otherwise (x86-64's cvttss2si of a 64-bit register);
  a channel is the low 32 bits of q; the pixel is (r << 16) + (g << 8) + b mod 2^32."""
import numpy as np

F32 = np.float32
INT64_MIN = np.int64(-2 ** 63)
ITS = [1, 2, 3, 7, 64, 1000, 16777217, -1, -5]


def channel(v):
    """one f32 channel (array) -> uint32, the cast of k_resolve / ResolvePixel"""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(v < F32(1), v, F32(1)).astype(F32)
        s = (F32(255) * m).astype(F32)
        inr = (s > F32(-9.2e18)) & (s < F32(9.2e18))
        q = np.where(inr, np.trunc(np.where(inr, s, F32(0))).astype(np.int64), INT64_MIN)
    return (q & np.int64(0xFFFFFFFF)).astype(np.uint32)


def resolve(rgba, it):
    """(..., >= 3) float32 accumulator values, iteration count it (an int, converted to f32 as C does) -> uint32 pixels (...)"""
    a = np.asarray(rgba, F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        v = a[..., :3] / F32(it)
    c = [channel(v[..., k]).astype(np.uint64) for k in range(3)]
    return (((c[0] << np.uint64(16)) + (c[1] << np.uint64(8)) + c[2]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _steps(v, n=8):
    """v and its n f32 neighbours on either side"""
    out = [F32(v)]
    lo = hi = F32(v)
    for _ in range(n):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return out


def _crossing(k):
    """the smallest f32 v with f32(255 v) >= k (k a float): where the scaled value reaches k"""
    v = F32(F32(k) / F32(255))
    with np.errstate(over="ignore"):
        while F32(255) * v >= F32(k):
            v = np.nextafter(v, F32(-np.inf))
        while F32(255) * v < F32(k):
            v = np.nextafter(v, F32(np.inf))
    return v


def _bits(u):
    return np.array(u, dtype=np.uint32).view(F32)


def crafted_values():
    """the edge values of the cast: every k/255 boundary, the specials, the negatives where the int64 branch switches, NaNs"""
    vals = []
    for k in range(256):
        vals += _steps(F32(k) / F32(255))
        vals += _steps(_crossing(k))
        vals += _steps(-_crossing(k))
    tiny = np.nextafter(F32(0), F32(1))
    fmax, fmin = np.finfo(F32).max, np.finfo(F32).tiny
    vals += [F32(0), F32(-0.0), tiny, fmin, F32(2), F32(1e30), fmax, F32(np.inf)]
    vals += _steps(F32(1))
    vals += [-tiny, F32(-1e-30), F32(-1) / F32(255), F32(-0.5), F32(-1), F32(-1e10), -fmax, F32(-np.inf)]
    # 255 v crosses +-9.2e18 (the f32 bounds of the int64 branch) near v = +-3.6e16
    for b in (F32(9.2e18), F32(-9.2e18)):
        vals += _steps(_crossing(b) if b > 0 else -_crossing(-b))
    vals += list(_bits([0x7FC00000, 0x7FC00001, 0x7FC12345, 0x7FFFFFFF, 0x7F800001, 0x7FA00000,
                        0xFFC00000, 0xFFC00001, 0xFFFFFFFF, 0xFF800001]))
    return np.array(vals, F32)


def value_set(n_random=1 << 20, seed=20261016):
    """crafted_values followed by n_random seeded bit patterns"""
    rnd = np.random.default_rng(seed).integers(0, 1 << 32, n_random, dtype=np.uint64).astype(np.uint32).view(F32)
    return np.concatenate([crafted_values(), rnd])


def pixels(values, n, seed=7):
    """n float4 pixels whose three channels walk the value list independently (r in order, g and b in seeded permutations), w random"""
    rng = np.random.default_rng(seed)
    reps = -(-n // len(values))
    out = np.empty((n, 4), F32)
    out[:, 0] = np.tile(values, reps)[:n]
    out[:, 1] = np.tile(values[rng.permutation(len(values))], reps)[:n]
    out[:, 2] = np.tile(values[rng.permutation(len(values))], reps)[:n]
    out[:, 3] = rng.standard_normal(n).astype(F32)
    return out
