"""Coordinate families shared by the lookup's forward and backward tests: Gaussian flows, the
integer grid, the lookup's edge cases, non-finite and huge values sprinkled over a flow, and the
integer grid displaced by single ulps (both sides of every floor decision)."""
import numpy as np

import prng


def _sprinkled(B, H, W):
    """A sigma = 3 flow with NaN, +-inf and huge coordinates over 64 entries."""
    c = prng.lookup_coords(314, B, H, W, 3.0)
    flat = c.reshape(-1)
    idx = (prng.uniform(315, (64,)) * flat.size).astype(np.int64)
    flat[idx] = np.resize(np.array([np.nan, np.inf, -np.inf, 3.0e38, -1e30, 1e6, -0.0, 2.0 ** 20], np.float32), 64)
    return c


def _ulps(v, u):
    """float32 v displaced by u units in its last place (towards +inf for u > 0)."""
    v = np.asarray(v, np.float32)
    u = np.broadcast_to(np.asarray(u, np.int32), v.shape)
    bits = v.view(np.int32)
    away = np.where(v > 0, bits + u, bits - u)                       # |bits| grows with |v|
    zero = np.where(u >= 0, u, np.int32(-2 ** 31) | (-u))            # around 0: +-|u| denormals
    return np.where(v == 0, zero, away).astype(np.int32).view(np.float32)


def _near_integer(B, H, W):
    """The integer grid displaced by 0, +-1, +-2, +-4 ... ulps and by +-2^-l fractions (every
    combination of the two cycles occurs once B * H * W >= 135), so that both sides of every floor
    decision of every level occur; then columns and rows just outside the map and values around
    +-2^20 * 2^l (the far sentinel's threshold at level l), each with its ulp neighbours, in the
    last queries of each axis' half of the map (x in the first half, y in the second)."""
    c = prng.coords_grid(B, H, W).reshape(B, 2, -1).copy()
    n = c.shape[-1]
    k = np.arange(n)
    ulps = np.array([0, 1, -1, 2, -2, 4, -4, 8, -8, 16, -16, 64, -64, 1024, -1024], np.int32)
    fracs = np.array([0, 0.125, -0.125, 0.25, -0.25, 0.5, -0.5, 1, -1], np.float32)
    for b in range(B):
        for a in range(2):
            v = c[b, a] + fracs[(k // len(ulps) + b + a * (k // 135)) % len(fracs)]   # exact in fp32
            c[b, a] = _ulps(v, ulps[(k + 3 * a + 5 * b) % len(ulps)])
    for a, size in ((0, W), (1, H)):
        edge = np.array([-1, -2, -0.5, size - 1, size - 0.5, size, size + 1, 2 * size], np.float32)
        big = np.array([s * (2.0 ** 20 * 2 ** l + d) for l in range(4) for d in (-1, 0, 1) for s in (1, -1)], np.float32)
        base = np.concatenate([edge, big])
        vals = np.concatenate([base, _ulps(base, 1), _ulps(base, -1), _ulps(base, 4), _ulps(base, -4)])
        m = min(len(vals), n // 2)
        hi = (a + 1) * (n // 2)
        c[:, a, hi - m:hi] = vals[:m]
    return c.reshape(B, 2, H, W).astype(np.float32)


def family_bwd_case(family, B, H, W, L, r, seed=400):
    """A backward case of two lookups (numpy): lookup 0 on the family's coordinates, lookup 1 on a
    sigma = 2 flow, so that the accumulation across lookups mixes window kinds; Gaussian upstream
    gradients [B, L * (2r+1)^2, H, W].  Returns (coords list, gradients list)."""
    K = (2 * r + 1) ** 2
    cs = [FAMILIES[family](B, H, W), prng.lookup_coords(seed, B, H, W, 2.0)]
    gs = [prng.gauss(seed + 10 + t, (B, L * K, H, W)) for t in range(len(cs))]
    return cs, gs


FAMILIES = {
    "sigma0": lambda B, H, W: prng.lookup_coords(311, B, H, W, 0.0),
    "sigma4": lambda B, H, W: prng.lookup_coords(312, B, H, W, 4.0),
    "sigma25": lambda B, H, W: prng.lookup_coords(313, B, H, W, 25.0),
    "grid": prng.coords_grid,
    "special": prng.special_coords,
    "sprinkled": _sprinkled,
    "near_integer": _near_integer,
}
