"""The lookup's backward (corr_lookup_bwd.hip) and the fused fold (corr_lookup_fold.hip) on the
coordinate families that pin the forward lookup (tests/_coords.py): Gaussian flows, the integer
grid, the grid displaced by single ulps and 2^-l fractions, denormals and -0.0, columns and rows
just outside the map, values on both sides of 2^20 * 2^l, NaN and infinities.  The irregular
window and sequential scatter paths of the fold exist for exactly these inputs.

Shapes: a 1x1 last level, level widths 20/10/5/2, odd sizes with a ragged last query group, an odd
H with W % 4 == 0 (the lean fold's unpooled last row), the radii 0, 1, 2 and 7 (16, 8, 8 and 2
queries per workgroup of the fold: FusedStage<S>::BQ depends on the radius alone), and query-row
slabs (NQ < H * W, one of them with a ragged last group).  Every case has two lookups, the
family's coordinates and then a sigma = 2 flow, so the accumulation across lookups mixes window
kinds.  D = 8: the GEMMs cost nothing.  The oracle's gradient pyramid of a case is the fp32 sum, in
lookup order, of oracle.lookup_bwd of each lookup from a zeroed pyramid, as autograd adds the
reference's per-lookup grid_sample gradients (one oracle.lookup_bwd call accumulating both
lookups corner by corner rounds otherwise and is no reference for T > 1).

Everything that follows the reference's order (the per-lookup kernel, the multi-lookup kernel, the
pool folds, corr_backward with the exact fold, every radius but 4) is compared bit for bit with
the fp32 oracle.  The separable fold (r = 4, exact=False: what training uses) rounds in another
order; its dC is held to the per-cell bound of tests/_util.py: |dC - oracle| <= k * (2^-24 * M +
2^-149) with M = sum |contribution| of the cell and k = 2 * (9 T L + L + 3), derived there, and
bit-equality wherever M = 0.

Observed on the MI355X, as information (the bound is the derived k, 150 at T = 2, L = 4 and 116
at L = 3, and is not tightened to this): the largest max |dC - oracle| / (2^-24 M) over the 68
separable-fold cases of this module is 4.822, at (1, 17, 23, 3, 4) with sigma4 on the whole map
(both algorithms: the fold does not depend on the GEMMs'); (3, 12, 20, 4, 4) sprinkled follows
with 4.813.  No case left an untouched cell (M = 0) other than +0.

The radius-7 cases found corr_lookup_bwd and corr_lookup_bwd_multi unusable at radius 7: 64
queries x 17 columns are 1088 threads, more than a workgroup's 1024, so every launch failed with
"invalid configuration argument"; the kernel now takes 32 queries per workgroup there.

Run on the GPU box: pytest -m gpu.
"""
import functools

import numpy as np
import pytest
import torch

import prng
from _coords import FAMILIES, family_bwd_case
from _util import bit_equal, cell_bound_k, cell_magnitude, cell_ratio, norm_rel, within_cell_bound
from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 8
T = 2

SHAPES = [
    (1, 8, 8, 4, 4),      # a 1x1 level; windows larger than every map; lean fold
    (3, 12, 20, 4, 4),    # level widths 20, 10, 5, 2
    (1, 17, 23, 3, 4),    # odd sizes, L = 3, a ragged last group of 3 queries; generic fold
    (2, 17, 20, 4, 4),    # odd H with W % 4 == 0: lean fold with an unpooled last row
    (1, 16, 24, 3, 0),    # radius 0: 16 queries per workgroup
    (1, 16, 24, 3, 1),    # radius 1: 8
    (1, 16, 24, 3, 2),    # radius 2: 8
    (1, 16, 24, 3, 7),    # radius 7: 2
]
SLABS = [
    ((1, 17, 23, 3, 4), (3, 8)),     # NQ = 115: a ragged last group of 3 queries
    ((2, 17, 20, 4, 4), (8, 17)),    # NQ = 180, down to the last query row
]
SLAB_FAMILIES = ["near_integer", "special", "sigma4"]
ALGOS = ["bf16x6", "f16x3"]


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from eraft_amd import _lib
    _lib.load()  # the HIP library must be the thing under test (no fallback exists)


def _dev(a):
    return torch.from_numpy(np.array(a, np.float32)).to(DEV)   # (a copy: the shared cases are read-only)


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _fmaps(B, H, W):
    return _frozen([prng.gauss(301, (B, D, H, W)), prng.gauss(302, (B, D, H, W))])


@functools.lru_cache(maxsize=None)
def _case(family, shape, rows=None):
    """The case's lookups (numpy coords and gradients; a query-row slab of them with `rows`) and
    the oracle's gradient pyramid before and after the pool backward, computed once and shared
    read-only by the tests."""
    B, H, W, L, r = shape
    cs, gs = family_bwd_case(family, B, H, W, L, r)
    if rows is not None:
        cs = [np.ascontiguousarray(c[:, :, rows[0]:rows[1]]) for c in cs]
        gs = [np.ascontiguousarray(g[:, :, rows[0]:rows[1]]) for g in gs]
    NQ = cs[0].shape[2] * W
    # each lookup's gradient from a zeroed pyramid, the lookups' pyramids then added in lookup
    # order: what autograd does with the reference's grid_sample backward, and what the kernels
    # do per cell (s = the lookup's contributions in scatter order, then G = G + s)
    gp = [np.zeros((B * NQ, 1, h, w), np.float32) for h, w in oracle.level_shapes(H, W, L)]
    for c, g in zip(cs, gs):
        one = oracle.lookup_bwd_rows(c, g, [np.zeros_like(p) for p in gp], H, W, r)
        gp = [p + s for p, s in zip(gp, one)]
    pre = [p.copy() for p in gp]
    oracle.pool_bwd(gp, H, W)
    return _frozen(cs), _frozen(gs), _frozen(pre), _frozen(gp)


@functools.lru_cache(maxsize=None)
def _magnitude(family, shape, rows=None):
    B, H, W, L, r = shape
    cs, gs, _, _ = _case(family, shape, rows)
    return _frozen([cell_magnitude(cs, gs, H, W, L, r)])[0]


def _grad_pyramid(shape, NQ=None, zero=False, nan=False):
    from eraft_amd.corr import _alloc_grad_pyramid
    B, H, W, L, _ = shape
    gl = _alloc_grad_pyramid(B, H, W, L, torch.empty(1, device=DEV), zero=zero, NQ=NQ)
    if nan:
        for p in gl:
            p.fill_(float("nan"))
    return gl


def _per_lookup(shape, cs, gs, NQ=None):
    """zero + corr_lookup_bwd per lookup: the slab's (or map's) gradient pyramid on the GPU."""
    from eraft_amd import _lib
    _, H, W, _, r = shape
    gl = _grad_pyramid(shape, NQ, zero=True)
    for c, g in zip(cs, gs):
        _lib.lookup_bwd(_dev(c), _dev(g), r, gl, H, W)
    return gl


def _assert_levels_equal(got, want, what):
    for l, (a, b) in enumerate(zip(got, want)):
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
        b = b.cpu().numpy() if isinstance(b, torch.Tensor) else b
        assert bit_equal(a, b), (what, l, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


# ---------------------------------------------------------------------------------------------
# a, b: the per-lookup kernel, the multi-lookup kernel and the two pool folds


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_lookup_bwd_vs_oracle(shape, family):
    """corr_lookup_bwd per lookup from a zeroed pyramid: every level bit-identical to the oracle's,
    and still so after corr_pool_bwd."""
    from eraft_amd import _lib
    _, H, W, _, _ = shape
    cs, gs, pre, post = _case(family, shape)
    gl = _per_lookup(shape, cs, gs)
    _assert_levels_equal(gl, pre, "lookup_bwd")
    _lib.pool_bwd(gl, H, W)
    _assert_levels_equal(gl, post, "pool_bwd")


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_lookup_bwd_multi_and_pool_fold(shape, family):
    """corr_lookup_bwd_multi into a NaN-filled pyramid equals the per-lookup result bit for bit
    (it overwrites every cell), and corr_pool_fold's level 0 equals corr_pool_bwd's."""
    from eraft_amd import _lib
    B, H, W, _, r = shape
    cs, gs, pre, post = _case(family, shape)
    ref = _per_lookup(shape, cs, gs)
    got = _grad_pyramid(shape, nan=True)
    _lib.lookup_bwd_multi([_dev(c) for c in cs], [_dev(g) for g in gs], r, got)
    _assert_levels_equal(got, ref, "multi vs per lookup")
    _assert_levels_equal(got, pre, "multi vs oracle")
    _lib.pool_bwd(ref, H, W)
    _lib.pool_fold(got, B, H, W)
    assert bit_equal(got[0].cpu().numpy(), ref[0].cpu().numpy())
    assert bit_equal(got[0].cpu().numpy(), post[0])


# ---------------------------------------------------------------------------------------------
# c, d, e: corr_backward on the whole map and on a query-row slab


def _staged_gemms(dc, f1, f2, algo):
    """The staged path's (dF1, dF2) on a given dC: corr_build_bwd_ex with its own maxima."""
    from eraft_amd import _lib
    B, _, H, W = f2.shape
    NQ = f1.shape[2] * f1.shape[3]
    return _lib.build_bwd(_dev(dc).reshape(B * NQ, H * W), f1, f2, _lib._ALGOS[algo])


def _run_backward(shape, cs, gs, f1, f2, algo, exact, NQ=None):
    from eraft_amd import _lib
    r = shape[4]
    got = _grad_pyramid(shape, NQ, nan=True)
    g1, g2 = _lib.backward([_dev(c) for c in cs], [_dev(g) for g in gs], r, got, f1, f2, _lib._ALGOS[algo],
                           exact=exact)
    return got[0].cpu().numpy(), g1.cpu().numpy(), g2.cpu().numpy()


def _check_backward(shape, family, algo, exact, rows=None):
    """corr_backward against the oracle's dC and the staged GEMMs on that dC.  exact, or a radius
    other than 4: everything bit-identical.  The separable fold: dC within the per-cell bound and
    with the oracle's non-finite pattern, dF1 and dF2 within the suite's 1e-6 norm-relative bar
    for this path, and a second run bit-identical to the first."""
    B, H, W, L, r = shape
    cs, gs, _, post = _case(family, shape, rows)
    f1n, f2n = _fmaps(B, H, W)
    f1 = _dev(f1n if rows is None else f1n[:, :, rows[0]:rows[1]])
    f2 = _dev(f2n)
    NQ = f1.shape[2] * W
    want = post[0]
    r1, r2 = (t.cpu().numpy() for t in _staged_gemms(want, f1, f2, algo))
    dc, g1, g2 = _run_backward(shape, cs, gs, f1, f2, algo, exact, NQ)
    if exact or r != 4:
        assert bit_equal(dc, want), int((dc.view(np.uint32) != want.view(np.uint32)).sum())
        assert bit_equal(g1, r1) and bit_equal(g2, r2)
        return None
    M = _magnitude(family, shape, rows)
    ratio = cell_ratio(dc, want, M)
    e1, e2 = norm_rel(g1, r1), norm_rel(g2, r2)
    assert np.array_equal(np.isfinite(dc), np.isfinite(want))
    print(f"{family} {shape} rows {rows} {algo}: max |dC - oracle| / (2^-24 M) = {ratio:.3f} "
          f"(k = {cell_bound_k(T, L)}), norm_rel dC {norm_rel(dc, want):.2e}, dF1 {e1:.2e}, dF2 {e2:.2e}")
    assert within_cell_bound(dc, want, M, T, L), ratio
    assert e1 <= 1e-6 and e2 <= 1e-6, (e1, e2)
    for a, b in zip((dc, g1, g2), _run_backward(shape, cs, gs, f1, f2, algo, exact, NQ)):
        assert bit_equal(a, b)
    return ratio


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_corr_backward_exact_fold(shape, family, algo):
    """corr_backward(exact=True): dC bit-identical to the oracle's, dF1 and dF2 bit-identical to
    the staged build_bwd on that dC."""
    _check_backward(shape, family, algo, True)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_corr_backward_default_fold(shape, family, algo):
    """corr_backward(exact=False), what training runs: at r = 4 the separable fold, held to the
    per-cell bound; at the other radii bit-identical."""
    _check_backward(shape, family, algo, False)


@pytest.mark.parametrize("family", SLAB_FAMILIES)
@pytest.mark.parametrize("shape,rows", SLABS, ids=str)
def test_slab_lookup_bwd_vs_oracle(shape, rows, family):
    """corr_lookup_bwd_rows and corr_pool_bwd on a query-row slab against oracle.lookup_bwd_rows
    and pool_bwd: bit-identical before and after the fold."""
    from eraft_amd import _lib
    _, H, W, _, _ = shape
    cs, gs, pre, post = _case(family, shape, rows)
    NQ = (rows[1] - rows[0]) * W
    gl = _per_lookup(shape, cs, gs, NQ)
    _assert_levels_equal(gl, pre, "lookup_bwd_rows")
    _lib.pool_bwd(gl, H, W)
    _assert_levels_equal(gl, post, "pool_bwd")


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("family", SLAB_FAMILIES)
@pytest.mark.parametrize("shape,rows", SLABS, ids=str)
def test_slab_corr_backward(shape, rows, family, algo, exact, monkeypatch):
    """corr_backward with NQ < H * W (what HipRows.backward runs) against the oracle's slab dC and
    the slab's staged build_bwd, as for the whole map; then HipRows.backward itself, which takes
    the algorithm and the fold from the environment, returns the same dF1 and partial dF2."""
    from eraft_amd.sharded import HipRows
    B, H, W, L, r = shape
    _check_backward(shape, family, algo, exact, rows)
    cs, gs, _, post = _case(family, shape, rows)
    f1n, f2n = _fmaps(B, H, W)
    f1, f2 = _dev(f1n[:, :, rows[0]:rows[1]]), _dev(f2n)
    monkeypatch.setenv("ERAFT_AMD_BUILD", algo)
    monkeypatch.setenv("ERAFT_AMD_EXACT_FOLD", "1" if exact else "0")
    h1, h2 = HipRows.backward([_dev(c) for c in cs], [_dev(g) for g in gs], r, f1, f2, L)
    assert h1.shape == f1.shape and h2.shape == f2.shape
    if exact:
        r1, r2 = _staged_gemms(post[0], f1, f2, algo)
    else:
        _, r1, r2 = _run_backward(shape, cs, gs, f1, f2, algo, exact, f1.shape[2] * W)
    for a, b in ((h1, r1), (h2, r2)):
        assert bit_equal(a.cpu().numpy(), b.cpu().numpy() if isinstance(b, torch.Tensor) else b)


# ---------------------------------------------------------------------------------------------
# f: the maxima that the fused fold hands to the f16x3 GEMMs


def _dominant_case(shape, which):
    """A sigma = 4 case in which one query's upstream gradient is scaled by 2^30 and every other
    one by 2^-10, the dominant query's window placed by `which`: over the last map row and column
    (a query in the middle of the list), in the last query group (the last query, its window in
    the middle of the map; ragged at 17 x 23), or over cell (0, 0) (the second query)."""
    B, H, W, L, r = shape
    cs, gs = family_bwd_case("sigma4", B, H, W, L, r, seed=440)
    n, (x, y) = {"last_row_col": (H * W // 2, (W - 1.25, H - 1.5)),
                 "last_group": (H * W - 1, (W / 2 + 0.25, H / 2 - 0.5)),
                 "cell_00": (1, (0.25, 0.5))}[which]
    b = B - 1
    for c, g in zip(cs, gs):
        c.reshape(B, 2, -1)[b, :, n] = (x, y)
        g *= np.float32(2.0 ** -10)
        g.reshape(B, g.shape[1], -1)[b, :, n] *= np.float32(2.0 ** 40)
    return cs, gs, b * H * W + n


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("which", ["last_row_col", "last_group", "cell_00"])
@pytest.mark.parametrize("shape", [(2, 17, 20, 4, 4), (1, 17, 23, 3, 4)], ids=str)
def test_fold_maxima_with_a_dominant_query(shape, which, algo, exact):
    """f16x3 takes dC's row and column maxima from the fused fold, not from a pass of its own; a
    maximum that misses the dominant cells overflows the f16 split and shows as inf or NaN.  With
    one query 2^40 above the others: exact, dC, dF1 and dF2 are bit-identical to the staged path,
    which computes its own maxima; otherwise they have the same (all-finite) pattern and are
    within the 1e-6 norm-relative bar."""
    from eraft_amd import _lib
    B, H, W, L, r = shape
    cs, gs, q = _dominant_case(shape, which)
    f1n, f2n = _fmaps(B, H, W)
    f1, f2 = _dev(f1n), _dev(f2n)
    ref = _per_lookup(shape, cs, gs)
    _lib.pool_bwd(ref, H, W)
    want = ref[0].cpu().numpy()
    # the dominant query's map holds the largest cells, on the place its window was put
    top = np.abs(want).reshape(B * H * W, H, W).max(axis=(1, 2))
    assert top.argmax() == q and top[q] > 2.0 ** 20 * np.delete(top, q).max()
    cells = np.abs(want.reshape(B * H * W, H, W)[q]) > 2.0 ** -10 * top[q]
    assert {"last_row_col": cells[H - 1, W - 1], "last_group": cells[H // 2, W // 2], "cell_00": cells[0, 0]}[which]
    r1, r2 = (t.cpu().numpy() for t in _lib.build_bwd(ref[0].reshape(B * H * W, H * W), f1, f2, _lib._ALGOS[algo]))
    assert np.isfinite(r1).all() and np.isfinite(r2).all()
    dc, g1, g2 = _run_backward(shape, cs, gs, f1, f2, algo, exact)
    if exact:
        assert bit_equal(dc, want) and bit_equal(g1, r1) and bit_equal(g2, r2)
    else:
        es = [norm_rel(a, b) for a, b in ((dc, want), (g1, r1), (g2, r2))]   # asserts the same finite pattern
        print(f"{shape} {which} {algo}: dC {es[0]:.2e}, dF1 {es[1]:.2e}, dF2 {es[2]:.2e}")
        assert max(es) <= 1e-6, es
