"""Correlation volumes past the 2^31 and 2^32 addressing marks, on an MI355X.

Every case of _large.CASES is the smallest shape of its geometry whose level 0 holds more than
2^31 (past-2^32: 2^32) words, so byte offsets past 2^31 and 2^32 and element indices past the
signed and the unsigned 32-bit range occur in the builds, the lookups and the backward.  Two legs:

  sampled  a few hundred query rows around every mark (and at batch boundaries) go to the host and
           are held to the C oracle, bit for bit wherever the suite does so at small sizes;
  dense    every word of the volume is checked on the device, in chunks of query rows: level 0
           against an fp64 matmul, the pooled levels against the oracle's sum order restated as
           tensor adds, the lookup / lookup_bwd / pool_bwd against the same entry point run on a
           fresh copy of the chunk (relocation: only the addresses differ), the backward GEMMs
           against fp64 matmuls over the kernel's own dC.

No level ever goes to the host.  Each test prints its wall time, its peak device memory and the
measured error / bound ratios ("LARGE ..." lines)."""
import contextlib
import functools
import gc
import time

import numpy as np
import pytest
import torch

import _large
import prng
from _large import CASES, D
from _util import REL_TOL, bit_equal, cell_bound_k, cell_magnitude, cell_ratio, norm_rel, within_cell_bound
from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = list(CASES)
TWO = ["one-map", "many-maps"]
CHUNK_WORDS = 2 ** 27  # words of level 0 per chunk of the dense legs (0.5 GB; its fp64 images 1 GB each)
GB = 2.0 ** 30


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from eraft_amd import _lib
    _lib.load()


@functools.lru_cache(maxsize=None)
def _host(case):
    """Features, planted coordinates (sigma = 3 cells) and the sampled queries of a case (numpy)."""
    c = CASES[case]
    B, H, W = c["B"], c["H"], c["W"]
    seed = 600 + 10 * ALL.index(case)
    f1, f2 = prng.gauss(seed, (B, D, H, W)), prng.gauss(seed + 1, (B, D, H, W))
    sample = _large.case_sample(case)
    coords = _large.plant_coords(prng.lookup_coords(seed + 2, B, H, W, 3.0), sample)
    return f1, f2, coords, sample


@contextlib.contextmanager
def _run(test, case, need_bytes):
    """Skip unless the device currently has need_bytes free; then time the body, record its peak
    memory, and give everything back before the next test allocates."""
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need_bytes:
        pytest.skip(f"{test}[{case}] needs {need_bytes / GB:.1f} GiB, the device has {free / GB:.1f} GiB free")
    torch.cuda.reset_peak_memory_stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    note = {}
    try:
        yield note
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device fault: nothing more of this file may start on the device
        if "HIP error" in str(e) or "[corr -3]" in str(e):
            pytest.exit(f"{test}[{case}]: the device reported {e}; the remaining tests are not run", returncode=3)
        raise
    finally:
        dt = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated()
        gc.collect()
        with contextlib.suppress(RuntimeError):
            torch.cuda.empty_cache()
        extra = " ".join(f"{k}={v}" for k, v in note.items())
        print(f"LARGE test={test} case={case} seconds={dt:.2f} peak_gib={peak / GB:.2f} {extra}")


def _dims(case):
    c = CASES[case]
    return c["B"], c["H"], c["W"], c["L"], c["r"], c["H"] * c["W"]


def _rows(case):
    """Query rows per chunk of the dense legs."""
    _, H, W, _, _, _ = _dims(case)
    return max(1, CHUNK_WORDS // _large.map_floats(H, W))


def _device(case):
    f1, f2, coords, sample = _host(case)
    t = [torch.from_numpy(a).to(DEV) for a in (f1, f2, coords)]
    return t[0], t[1], t[2], torch.from_numpy(sample).to(DEV)


def _flat(t):
    """[B, C, H, W] -> [C, B * H * W]: channel rows over flat queries."""
    return t.permute(1, 0, 2, 3).reshape(t.shape[1], -1)


def _slab(xf, q0, q1, NQ):
    """Flat queries [q0, q1) of xf [C, B * NQ] as the relocated call's [Bs, C, n, 1]: a row range of
    one batch item (Bs = 1) or whole batch items (n = NQ), as _large.chunks cuts them."""
    Bs = max(1, (q1 - q0) // NQ) if q1 - q0 > NQ else 1
    return xf[:, q0:q1].reshape(xf.shape[0], Bs, -1).permute(1, 0, 2).contiguous().unsqueeze(-1)


def _build(case, t1, t2, algo="bf16x6"):
    from eraft_amd import _lib
    from eraft_amd.corr import _alloc_pyramid
    B, H, W, L, _, _ = _dims(case)
    lv = _alloc_pyramid(B, H, W, L, t1)
    _lib.build(t1, t2, lv, _lib._ALGOS[algo])
    return lv


def _export_rows(lv, idx, H, W):
    """The sampled query rows of the tiled levels, in the reference's layout, on the host."""
    from eraft_amd import _lib
    return [p.cpu().numpy() for p in _lib.pyramid_export([p[idx] for p in lv], H, W)]


def _upstream(case, seed, only=None):
    """Upstream gradients [B, L * K, H, W] made on the device (too many for the host generator);
    only: zero outside these flat queries."""
    B, H, W, L, r, NQ = _dims(case)
    LK = L * (2 * r + 1) ** 2
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    if only is None:
        return torch.randn((B, LK, H, W), generator=gen, device=DEV)
    g = torch.zeros((B, LK, NQ), device=DEV)
    g[only // NQ, :, only % NQ] = torch.randn((only.numel(), LK), generator=gen, device=DEV)
    return g.view(B, LK, H, W)


def _staged_dc(case, coords_list, grads_list, keep_pre=False):
    """The staged path's gradient pyramid: zero, lookup_bwd per lookup, pool_bwd (level 0 = dC).
    keep_pre: also a copy of the pyramid before pool_bwd."""
    from eraft_amd import _lib
    from eraft_amd.corr import _alloc_grad_pyramid
    B, H, W, L, r, _ = _dims(case)
    gl = _alloc_grad_pyramid(B, H, W, L, coords_list[0], zero=True)
    for c, g in zip(coords_list, grads_list):
        _lib.lookup_bwd(c, g, r, gl)
    pre = [p.clone() for p in gl] if keep_pre else None
    _lib.pool_bwd(gl, H, W)
    return gl, pre


def _oracle_dc_rows(case, cf, gf, idx):
    """The oracle's gradient pyramid rows of the sampled queries, before and after pool_bwd:
    cf / gf lists of flat coords [2, BN] / gradients [LK, BN] on the device."""
    B, H, W, L, r, _ = _dims(case)
    n = idx.numel()
    gp = [np.zeros((n, 1, h, w), np.float32) for h, w in oracle.level_shapes(H, W, L)]
    cs, gs = [], []
    for c, g in zip(cf, gf):
        cs.append(c[:, idx].cpu().numpy()[None, :, :, None])
        gs.append(g[:, idx].cpu().numpy()[None, :, :, None])
        oracle.lookup_bwd_rows(cs[-1], gs[-1], gp, H, W, r)
    pre = [p.copy() for p in gp]
    oracle.pool_bwd(gp, H, W)
    return pre, gp, cs, gs


# --------------------------------------------------------------------------------------------
# build: level 0 and the pooled levels
# --------------------------------------------------------------------------------------------
def _build_body(case, algo, note):
    from eraft_amd import _lib
    B, H, W, L, r, NQ = _dims(case)
    f1, f2, _, sample = _host(case)
    t1, t2, _, idx = _device(case)
    lv = _build(case, t1, t2, algo)
    # sampled rows against the oracle
    rows = _export_rows(lv, idx, H, W)
    S = (D + 31) // 32
    worst_rel = worst_el = 0.0
    for k, qi in enumerate(sample):
        b, n = divmod(int(qi), NQ)
        ref = oracle.corr_rows(f1[b:b + 1], f2[b:b + 1], n, n + 1)[0, 0]
        got = rows[0][k, 0].ravel()
        worst_rel = max(worst_rel, norm_rel(got, ref))
        if algo == "bf16x6":  # test_build_bf16x6_error_bound's element-wise bound
            a = f1[b].reshape(D, NQ).astype(np.float64)[:, n]
            t = f2[b].reshape(D, NQ).astype(np.float64)
            ref64, mag = (a @ t) / np.sqrt(np.float64(D)), (np.abs(a) @ np.abs(t)) / np.sqrt(np.float64(D))
            bound = (3 + 6 * S) * 2.0 ** -24 * mag
            err = np.abs(got.astype(np.float64) - ref64)
            assert (err <= bound).all(), qi
            worst_el = max(worst_el, float((err / np.maximum(bound, 1e-300)).max()))
    note["sampled_rel"] = f"{worst_rel:.2e}"
    note["sampled_bound_ratio"] = f"{worst_el:.3f}"
    assert worst_rel < REL_TOL
    for l in range(1, L):
        assert bit_equal(oracle.avg_pool2x2(rows[l - 1]), rows[l]), l
    # every word on the device
    ratio, pooled = _large.sweep_level0(lambda q0, q1: _lib.pyramid_export([p[q0:q1] for p in lv], H, W),
                                        t1.view(B, D, NQ), t2.view(B, D, NQ), B, NQ, _rows(case), algo, REL_TOL)
    note["dense_ratio"] = f"{ratio:.3f}"
    assert pooled, "a pooled level differs from avg_pool2x2 of the level below"
    assert ratio <= 1.0 if algo == "bf16x6" else ratio < 1.0, ratio


@pytest.mark.parametrize("case,algo", [(c, "bf16x6") for c in ALL] + [(c, a) for c in TWO for a in ("f16x3", "fp32")])
def test_build_every_word(case, algo):
    """Level 0 of the build against the oracle (sampled rows, REL_TOL per row; bf16x6 also within
    its element-wise bound) and against fp64 on the device (every word: bf16x6 element-wise,
    (3 + 6 ceil(D / 32)) 2^-24 sum |a||b| / sqrt(D); f16x3 and fp32 REL_TOL per row); the pooled
    levels bit for bit against avg_pool2x2 of the level below, on the sample by the oracle and on
    every word by its restated sum order."""
    _host(case)
    with _run("build_" + algo, case, 1.25 * _large.pyramid_bytes(case, True) + 12 * GB) as note:
        _build_body(case, algo, note)


def _export_body(case):
    from eraft_amd import _lib
    B, H, W, L, r, NQ = _dims(case)
    t1, t2, _, _ = _device(case)
    lv = _build(case, t1, t2)
    full = _lib.pyramid_export(lv, H, W)
    for c in _large.chunks(B, NQ, _rows(case)):
        q0, q1 = _large.flat_range(c, NQ)
        part = _lib.pyramid_export([p[q0:q1] for p in lv], H, W)
        for l in range(L):
            assert _large.same_bits(full[l][q0:q1], part[l]), (q0, q1, l)


def test_whole_level_export():
    """pyramid_export of whole levels (many-maps: 2^31.1 words in, 2^31.04 out) gives the bits of
    the chunked exports that the other tests read the volume through."""
    case = "many-maps"
    with _run("export", case, _large.pyramid_bytes(case, True) + _large.pyramid_bytes(case, False) + 12 * GB):
        _export_body(case)


# --------------------------------------------------------------------------------------------
# lookup, lookup_conv
# --------------------------------------------------------------------------------------------
def _lookup_out(case, lv, c):
    from eraft_amd import _lib
    B, H, W, L, r, _ = _dims(case)
    out = torch.empty((B, L * (2 * r + 1) ** 2, H, W), device=DEV)
    _lib.lookup(lv, c, r, out)
    return out


def _lookup_body(case, note):
    from eraft_amd import _lib
    B, H, W, L, r, NQ = _dims(case)
    LK = L * (2 * r + 1) ** 2
    t1, t2, c, idx = _device(case)
    lv = _build(case, t1, t2)
    of, cf = _flat(_lookup_out(case, lv, c)), _flat(c)
    note["variant"] = f"QB{16 if H * W <= 2048 and B * NQ >= 20000 else 32},TIGHT{int(B * NQ >= 18000)}"
    # sampled queries against the oracle on the exported rows
    rows = _export_rows(lv, idx, H, W)
    cs = cf[:, idx].cpu().numpy()[None, :, :, None]
    assert np.isnan(cs).any() and np.isinf(cs).any()
    ref = oracle.lookup_rows(rows, cs, H, W, r).reshape(LK, -1)
    assert bit_equal(of[:, idx].cpu().numpy(), ref)

    def small(q0, q1):  # the chunk's rows in a fresh small pyramid, as a query slab
        cc = _slab(cf, q0, q1, NQ)
        out = torch.empty((cc.shape[0], LK, cc.shape[2], 1), device=DEV)
        _lib.lookup([p[q0:q1].clone() for p in lv], cc, r, out, H=H, W=W)
        return _flat(out)

    assert _large.sweep_relocated(B, NQ, _rows(case), lambda q0, q1: of[:, q0:q1], small) == []


@pytest.mark.parametrize("case", ALL)
def test_lookup_every_query(case):
    """The lookup of the whole volume: the sampled queries (special, integer-grid, NaN and inf
    coordinates planted among them) bit for bit against the oracle on their exported rows; every
    query bit for bit against the same entry point on a relocated copy of its chunk."""
    _host(case)
    with _run("lookup", case, 1.3 * _large.pyramid_bytes(case, True) + 12 * GB) as note:
        _lookup_body(case, note)


def _lookup_conv_body(case, note):
    import torch.nn.functional as F
    from eraft_amd import _lib
    B, H, W, L, r, NQ = _dims(case)
    LK = L * (2 * r + 1) ** 2
    t1, t2, c, _ = _device(case)
    lv = _build(case, t1, t2)
    lk = _lookup_out(case, lv, c)
    w = torch.from_numpy(prng.gauss(84, (256, LK, 1, 1), 0.05)).to(DEV)
    bias = torch.from_numpy(prng.gauss(85, (256,), 0.1)).to(DEV)
    pack = _lib.lookup_conv_weights(w)
    for relu in (True, False):
        out = torch.empty((B, 256, H, W), device=DEV)
        _lib.lookup_conv(lv, c, r, pack, bias, out, relu)
        diff = top = 0.0
        for b in range(B):
            ref = F.conv2d(lk[b:b + 1].double(), w.double(), bias.double())
            ref = torch.relu(ref) if relu else ref
            fin = torch.isfinite(ref)
            assert torch.equal(torch.isfinite(out[b:b + 1]), fin), (relu, b)
            diff = max(diff, float((out[b:b + 1].double() - ref)[fin].abs().max()))
            top = max(top, float(ref[fin].abs().max()))
        note[f"relu{int(relu)}"] = f"{diff / top:.2e}"
        assert diff <= 1e-5 * top, relu


def test_lookup_conv_many_maps():
    """corr_lookup_conv on many-maps against a torch 1x1 convolution (fp64) of the lookup that
    test_lookup_every_query checks: |diff| <= 1e-5 of the largest output, with and without ReLU."""
    case = "many-maps"
    _host(case)
    with _run("lookup_conv", case, _large.pyramid_bytes(case, True) + 12 * GB) as note:
        _lookup_conv_body(case, note)


# --------------------------------------------------------------------------------------------
# backward: lookup_bwd, pool_bwd, the GEMMs; corr_backward
# --------------------------------------------------------------------------------------------
def _check_gemms(case, dc, t1, t2, results, note, tag):
    """dF1 / dF2 of `results` {name: (dF1, dF2)} against fp64 matmuls over dC [BN, 1, H, W]."""
    B, H, W, L, r, NQ = _dims(case)
    r1, r2 = _large.gemm_reference(lambda q0, q1: dc[q0:q1].view(q1 - q0, NQ), t1.view(B, D, NQ), t2.view(B, D, NQ),
                                   B, NQ, _rows(case))
    for name, (d1, d2) in results.items():
        e1, e2 = _large.norm_rel_t(d1, r1), _large.norm_rel_t(d2, r2)
        note[f"{tag}_{name}"] = f"{e1:.1e}/{e2:.1e}"
        assert e1 < REL_TOL and e2 < REL_TOL, (name, e1, e2)


def _staged_body(case, note):
    from eraft_amd import _lib
    from eraft_amd.corr import _alloc_grad_pyramid
    B, H, W, L, r, NQ = _dims(case)
    LK = L * (2 * r + 1) ** 2
    t1, t2, c, idx = _device(case)
    g = _upstream(case, 7)
    cf, gf = _flat(c), _flat(g)
    gl, pre = _staged_dc(case, [c], [g], keep_pre=True)
    pool_cells = B * NQ * (2 * (H // 2)) * (2 * (W // 2))
    note["pool_bwd_index"] = "size_t" if pool_cells + 32768 * 256 >= 2 ** 32 else "unsigned"
    # sampled rows against the oracle: before and after pool_bwd, bit for bit
    opre, opost, _, _ = _oracle_dc_rows(case, [cf], [gf], idx)
    for l in range(L):
        assert bit_equal(pre[l][idx].cpu().numpy(), opre[l]), l
        assert bit_equal(gl[l][idx].cpu().numpy(), opost[l]), l
    assert np.count_nonzero(opost[0]) > 0

    def fresh(q0, q1):
        Bs = max(1, (q1 - q0) // NQ)
        return _alloc_grad_pyramid(Bs, H, W, L, c, zero=True, NQ=(q1 - q0) // Bs)

    def small_lookup_bwd(q0, q1):
        sg = fresh(q0, q1)
        _lib.lookup_bwd(_slab(cf, q0, q1, NQ), _slab(gf, q0, q1, NQ), r, sg, H=H, W=W)
        return sg

    def small_pool_bwd(q0, q1):
        sg = fresh(q0, q1)
        for s, p in zip(sg, pre):
            s.copy_(p[q0:q1])
        _lib.pool_bwd(sg, H, W)
        return sg

    assert _large.sweep_relocated(B, NQ, _rows(case), lambda q0, q1: [p[q0:q1] for p in pre], small_lookup_bwd) == []
    assert _large.sweep_relocated(B, NQ, _rows(case), lambda q0, q1: [p[q0:q1] for p in gl], small_pool_bwd) == []
    del pre
    if case in TWO or case == "tiny-maps":  # past-2^32 stops at the gradient pyramid
        algos = ("bf16x6", "f16x3", "fp32") if case in TWO else ("bf16x6",)
        res = {a: _lib.build_bwd(gl[0].view(B * NQ, NQ), t1, t2, _lib._ALGOS[a]) for a in algos}
        _check_gemms(case, gl[0], t1, t2, res, note, "dF")


@pytest.mark.parametrize("case", ALL)
def test_staged_backward_every_word(case):
    """lookup_bwd then pool_bwd over the whole gradient pyramid: the sampled rows bit for bit
    against the oracle, every word bit for bit against the same entry points on relocated chunks
    (pool_bwd's 64-bit index kernel on past-2^32); then build_bwd's dF1 / dF2 for each algorithm
    against fp64 matmuls over that dC at REL_TOL."""
    _host(case)
    with _run("staged_bwd", case, 2.2 * _large.pyramid_bytes(case, False) + 12 * GB) as note:
        _staged_body(case, note)


def _fused_body(case, algo, exact, note):
    from eraft_amd import _lib
    from eraft_amd.corr import _alloc_grad_pyramid
    B, H, W, L, r, NQ = _dims(case)
    t1, t2, c, idx = _device(case)
    g = _upstream(case, 7)
    ref, _ = _staged_dc(case, [c], [g])
    got = _alloc_grad_pyramid(B, H, W, L, c)
    got[0].fill_(float("nan"))  # corr_backward must overwrite every word of dC
    res = _lib.backward([c], [g], r, got, t1, t2, _lib._ALGOS[algo], exact=exact)
    lds_fold = case == "tiny-maps"  # the LDS-resident fused fold; larger maps take multi + pool_fold
    note["fold"] = ("fused-lds" if lds_fold else "multi+pool_fold") + ("-exact" if exact else "")
    if exact or not lds_fold:  # bit-identical, as test_corr_backward_matches_staged_path holds them
        for q0 in range(0, B * NQ, _rows(case)):
            q1 = min(B * NQ, q0 + _rows(case))
            assert _large.same_bits(got[0][q0:q1], ref[0][q0:q1]), (q0, q1)
    else:
        d = s = 0.0
        for q0 in range(0, B * NQ, _rows(case)):
            q1 = min(B * NQ, q0 + _rows(case))
            a, b = got[0][q0:q1], ref[0][q0:q1]
            assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
            d, s = max(d, float((a - b).abs().max())), max(s, float(b.abs().max()))
        note["dC_norm_rel"] = f"{d / s:.2e}"
        assert d / s <= 1e-6
        # the separable fold did run: a fall-back to multi + pool_fold would give the staged bits
        assert d > 0, "corr_backward's default fold gave the staged path's bits: the fused fold did not run"
        # the per-cell bound over every word: M is the staged path on |g| (the kernels that
        # test_staged_backward_every_word holds to the oracle bit for bit), as _util.cell_magnitude
        Mg, _ = _staged_dc(case, [c], [g.abs()])
        ok, worst = _large.cell_bound_sweep(*[lambda q0, q1, v=v: v[0][q0:q1] for v in (got, ref, Mg)],
                                            cell_bound_k(1, L), B, NQ, _rows(case))
        note["dense_cell_ratio"] = f"{worst:.3f}/{cell_bound_k(1, L)}"
        assert ok
        del Mg
    # the sampled rows: the exact fold is the oracle's bits, the default within the per-cell bound
    _, opost, cs, gs = _oracle_dc_rows(case, [_flat(c)], [_flat(g)], idx)
    rows = got[0][idx].cpu().numpy()
    if exact or not lds_fold:
        assert bit_equal(rows, opost[0])
    else:
        M = cell_magnitude(cs, gs, H, W, L, r)
        note["cell_ratio"] = f"{cell_ratio(rows, opost[0], M):.3f}/{cell_bound_k(1, L)}"
        assert within_cell_bound(rows, opost[0], M, 1, L)
    del ref
    _check_gemms(case, got[0], t1, t2, {algo: res}, note, "dF")


@pytest.mark.parametrize("case,algo,exact", [(c, "bf16x6", e) for c in ALL[:3] for e in (True, False)] +
                         [(c, a, False) for c in TWO for a in ("f16x3", "fp32")])
def test_fused_backward_every_word(case, algo, exact):
    """corr_backward against the staged path as test_corr_backward_matches_staged_path compares
    them (bit-identical dC with the exact fold and on the multi-lookup + pool_fold path of the maps
    too large for LDS; the LDS-resident separable fold of tiny-maps within 1e-6 norm-relative,
    different from the staged bits somewhere (so the fused fold is what ran), and within the
    per-cell bound: on every word with M from the staged kernels on |g|, on the sampled rows with
    the oracle's M), the sampled dC rows against the oracle, and its dF1 / dF2 against fp64 matmuls
    over its own dC at REL_TOL.  The other variants named in the LARGE lines (lookup QB / TIGHT,
    pool_bwd's index type, multi + pool_fold) are restated from the launch conditions, not observed."""
    _host(case)
    with _run(f"fused_bwd_{algo}_{'exact' if exact else 'default'}", case,
              3.3 * _large.pyramid_bytes(case, False) + 12 * GB) as note:
        _fused_body(case, algo, exact, note)


def _untouched_body(case, note):
    from eraft_amd import _lib
    from eraft_amd.corr import _alloc_grad_pyramid
    B, H, W, L, r, NQ = _dims(case)
    t1, t2, c, idx = _device(case)
    g = _upstream(case, 9, only=idx)
    paths = {"staged": _staged_dc(case, [c], [g])[0]}
    if case != "past-2^32":
        got = _alloc_grad_pyramid(B, H, W, L, c)
        for p in got:
            p.fill_(float("nan"))
        _lib.backward([c], [g], r, got, t1, t2, _lib._ALGOS["bf16x6"], exact=False)
        paths["fused"] = got
    for name, gl in paths.items():
        counts = _large.count_nonzero_rows(lambda q0, q1: gl[0][q0:q1], B, NQ, _rows(case))
        inside, total = int(counts[idx].sum()), int(counts.sum())
        note[name] = f"{inside}/{total}"
        assert total == inside > 0, name


@pytest.mark.parametrize("case", ALL)
def test_untouched_cells_stay_zero(case):
    """With upstream gradients that are zero outside the sampled queries, the nonzero words of dC
    over the whole volume are those inside the sampled rows: no store lands in another row (staged
    path; corr_backward from a NaN-filled scratch pyramid too)."""
    _host(case)
    with _run("untouched", case, 2.2 * _large.pyramid_bytes(case, False) + 12 * GB) as note:
        _untouched_body(case, note)


def _corrblock_body(case, note, monkeypatch):
    from eraft_amd import CorrBlock, _lib
    B, H, W, L, r, NQ = _dims(case)
    t1, t2, c, idx = _device(case)
    cs = [c, c + 0.37]
    gs = [_upstream(case, 11), _upstream(case, 12)]
    kept = {}
    fused = _lib.backward

    def spy(coords_list, grad_list, radius, grad_levels, *a, **k):
        kept["dc"] = grad_levels[0]
        return fused(coords_list, grad_list, radius, grad_levels, *a, **k)
    monkeypatch.setattr(_lib, "backward", spy)
    monkeypatch.setenv("ERAFT_AMD_FUSED_BWD", "1")
    monkeypatch.setenv("ERAFT_AMD_EXACT_FOLD", "0")
    monkeypatch.setenv("ERAFT_AMD_BUILD", "bf16x6")
    a1, a2 = t1.clone().requires_grad_(True), t2.clone().requires_grad_(True)
    cb = CorrBlock(a1, a2, num_levels=L, radius=r)
    outs = [cb(x) for x in cs]
    lv = cb._state.levels
    for x, o in zip(cs, outs):  # the public lookups are the entry point's
        assert _large.same_bits(o.detach(), _lookup_out(case, lv, x))
    sum((o * g).sum() for o, g in zip(outs, gs)).backward()
    del outs, cb, lv
    ref, _ = _staged_dc(case, cs, gs)
    for q0 in range(0, B * NQ, _rows(case)):  # 181x257 maps: multi + pool_fold, the staged path's bits
        q1 = min(B * NQ, q0 + _rows(case))
        assert _large.same_bits(kept["dc"][q0:q1], ref[0][q0:q1]), (q0, q1)
    del ref
    _check_gemms(case, kept["dc"], t1, t2, {"autograd": (a1.grad, a2.grad)}, note, "dF")


def test_corrblock_autograd_one_map(monkeypatch):
    """The public CorrBlock under autograd on one-map: build, two lookups, loss.backward().  The
    lookups are the entry point's bits, the dC that corr_backward leaves is the staged path's, and
    fmap1.grad / fmap2.grad go against fp64 matmuls over that dC at REL_TOL."""
    case = "one-map"
    _host(case)
    with _run("corrblock", case, _large.pyramid_bytes(case, True) + 2.2 * _large.pyramid_bytes(case, False) + 12 * GB) as note:
        _corrblock_body(case, note, monkeypatch)
