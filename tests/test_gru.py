"""The fused SepConvGRU half step (corr_gru_*, eraft_amd/gru.py, csrc/corr_gru.hip).

CPU: the exports, the size functions and the argument validation (all before any HIP call), and
that the module switch is inert on CPU tensors.  GPU: parity of the half step with an fp64 CPU
evaluation of the same formulas within REL_TOL (norm-relative), direction / tap order, the
reference's own SepConvGRU (tests/golden/gru_reference.npz, make_golden_gru.py), determinism, graph
capture, re-packing, the module switch and the end-to-end golden.

Measured on an MI355X (norm_rel against fp64; torch's own fp32 GPU chain beside it): see
DESIGN.md §14.
"""
import copy
import functools
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prng
from _util import REL_TOL, bit_equal, load, norm_rel

HID = 128
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
NAMES = ("corr_gru_weights_bytes", "corr_gru_pack_weights", "corr_gru_workspace", "corr_gru_half_step")


# ----------------------------------------------------------------------------------------------
# shared data
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(inp, tag):
    """(wz, wr, wq) [128, C, 5] and (bz, br, bq) [128] of half step `tag`, from prng.param_init by
    parameter name (float32 numpy; read-only by convention)."""
    C = HID + inp
    shape = (HID, C, 1, 5) if tag == "1" else (HID, C, 5, 1)
    ws = tuple(prng.param_init(f"conv{g}{tag}.weight", shape).reshape(HID, C, 5) for g in "zrq")
    bs = tuple(prng.param_init(f"conv{g}{tag}.bias", (HID,)) for g in "zrq")
    return ws, bs


@functools.lru_cache(maxsize=None)
def _inputs(seed, B, inp, H, W):
    h = np.tanh(prng.gauss(seed, (B, HID, H, W)).astype(np.float64)).astype(np.float32)
    return h, prng.gauss(seed + 1, (B, inp, H, W))


def _chain(h, x, ws, bs, d):
    """One half step in the tensors' own dtype / device: the formulas of update.py:45-60."""
    shp, pad = ((1, 5), (0, 2)) if d == 0 else ((5, 1), (2, 0))
    conv = lambda w, b, t: F.conv2d(t, w.reshape(w.shape[0], w.shape[1], *shp), b, padding=pad)
    hx = torch.cat([h, x], 1)
    z = torch.sigmoid(conv(ws[0], bs[0], hx))
    r = torch.sigmoid(conv(ws[1], bs[1], hx))
    q = torch.tanh(conv(ws[2], bs[2], torch.cat([r * h, x], 1)))
    return (1 - z) * h + z * q


def _to(arrs, dev, dtype):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype) for a in arrs)


def _ref64(h, x, ws, bs, d):
    (h64, x64), w64, b64 = _to((h, x), "cpu", torch.float64), _to(ws, "cpu", torch.float64), _to(bs, "cpu", torch.float64)
    return _chain(h64, x64, w64, b64, d).numpy()


def _fused(h, x, ws, bs, d, dev="cuda:0"):
    from eraft_amd import _lib
    (hg, xg), wg, bg = _to((h, x), dev, torch.float32), _to(ws, dev, torch.float32), _to(bs, dev, torch.float32)
    shp = (1, 5) if d == 0 else (5, 1)
    packed = _lib.gru_pack_weights(*(w.reshape(HID, -1, *shp) for w in wg))
    return _lib.gru_half_step(hg, xg, d, packed, *bg).cpu().numpy()


def _module(inp=320, dev="cpu"):
    from eraft_amd.model import SepConvGRU
    m = SepConvGRU(hidden_dim=HID, input_dim=inp).eval()
    with torch.no_grad():
        for name, t in m.state_dict().items():
            t.copy_(torch.from_numpy(prng.param_init(name, tuple(t.shape))))
    return m.to(dev)


def _module64(m, h, x):
    m64 = copy.deepcopy(m).cpu().double()
    with torch.no_grad():
        return m64(torch.from_numpy(h).double(), torch.from_numpy(x).double()).numpy()


# ----------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from eraft_amd.build import build_library
    from eraft_amd import _lib
    build_library()
    return _lib.load()


def test_exports(lib):
    from eraft_amd import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name


def test_sizes(lib):
    align = lambda n: (n + 255) // 256 * 256
    for B, H, W in ((1, 60, 80), (2, 7, 9), (1, 1, 1)):
        assert lib.corr_gru_workspace(B, HID, H, W) == 2 * align(B * HID * H * W * 4)
        assert lib.corr_gru_workspace(B, HID, H, W) == 2 * B * HID * H * W * 4
    for bad in ((0, HID, 60, 80), (1, 0, 60, 80), (1, HID, 0, 80), (1, HID, 60, -1)):
        assert lib.corr_gru_workspace(*bad) == 0
    for inp in (320, 32, 896):
        assert lib.corr_gru_weights_bytes(HID, inp) >= 3 * HID * 5 * (HID + inp) * 6
    assert lib.corr_gru_weights_bytes(64, 320) == 0 and lib.corr_gru_weights_bytes(HID, 321) == 0


# corr_gru_half_step(h, x, B, hidden, input, H, W, dir, packed, bz, br, bq, ws, ws_bytes, h_out, stream)
_GOOD = dict(h=0x1000, x=0x2000, B=1, hidden=HID, input=320, H=6, W=7, dir=0, packed=0x3000, bz=0x4000, br=0x5000,
             bq=0x6000, ws=0x7000, ws_bytes=2 * HID * 42 * 4, h_out=0x8000, stream=None)


@pytest.mark.parametrize("change,code,msg", [
    (dict(hidden=64), EUNSUPPORTED, "hidden = 128"),
    (dict(hidden=256), EUNSUPPORTED, "hidden = 128"),
    (dict(input=321), EUNSUPPORTED, "multiple of 32"),
    (dict(input=1024), EUNSUPPORTED, "<= 1024"),
    (dict(h=None), EINVAL, "h is NULL"),
    (dict(packed=None), EINVAL, "packed is NULL"),
    (dict(h_out=None), EINVAL, "h_out is NULL"),
    (dict(dir=2), EINVAL, "dir must be"),
    (dict(dir=-1), EINVAL, "dir must be"),
    (dict(packed=0x3004), EINVAL, "packed is not 16-byte aligned"),
    (dict(ws_bytes=2 * HID * 42 * 4 - 1), EINVAL, "workspace of"),
    (dict(ws=None), EINVAL, "workspace of"),
    (dict(h_out=0x1000), EINVAL, "alias"),
    (dict(B=0), EINVAL, "B, H, W"),
])
def test_half_step_validation(lib, change, code, msg):
    """Every refusal comes before any HIP call (the pointers are never dereferenced)."""
    a = dict(_GOOD, **change)
    assert lib.corr_gru_half_step(*a.values()) == code
    assert msg in lib.corr_last_error().decode()


def test_pack_validation(lib):
    assert lib.corr_gru_pack_weights(16, 16, 16, 64, 320, 16, None) == EUNSUPPORTED
    assert lib.corr_gru_pack_weights(16, 16, 16, HID, 100, 16, None) == EUNSUPPORTED
    assert lib.corr_gru_pack_weights(16, None, 16, HID, 320, 16, None) == EINVAL
    assert "wr is NULL" in lib.corr_last_error().decode()
    assert lib.corr_gru_pack_weights(16, 16, 16, HID, 320, 20, None) == EINVAL
    assert "aligned" in lib.corr_last_error().decode()


def test_module_switch_is_inert_on_cpu(monkeypatch):
    from eraft_amd.model import SepConvGRU
    m = _module(32)
    h, x = (torch.from_numpy(a) for a in _inputs(3, 1, 32, 6, 7))
    with torch.no_grad():
        monkeypatch.setattr(SepConvGRU, "fused", False)
        a = m(h, x)
        monkeypatch.setattr(SepConvGRU, "fused", True)
        b = m(h, x)
    assert bit_equal(a.numpy(), b.numpy())


def test_sepconv_gru_refuses_cpu_tensors():
    from eraft_amd.gru import sepconv_gru
    h, x = (torch.from_numpy(a) for a in _inputs(3, 1, 32, 6, 7))
    with pytest.raises(RuntimeError, match="MI355X"):
        sepconv_gru(_module(32), h, x)


def test_switch_follows_the_environment_and_defaults_to_off():
    import os
    from eraft_amd.model import SepConvGRU
    assert SepConvGRU.fused is (os.environ.get("ERAFT_AMD_FUSE_GRU", "0") == "1")


# ----------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("B,H,W,inp", [
    (1, 1, 1, 320),    # every tap but the centre is padding
    (1, 3, 4, 320),    # the halo covers the whole map
    (2, 7, 9, 320),    # odd sizes, partial tiles, B > 1
    (1, 5, 70, 320),   # more than two tiles along W
    (1, 70, 5, 320),   # more than two tiles along H
    (2, 7, 9, 32),     # C = 160
])
def test_half_step_parity(B, H, W, inp, d):
    ws, bs = _weights(inp, "12"[d])
    h, x = _inputs(11 + d, B, inp, H, W)
    ref = _ref64(h, x, ws, bs, d)
    got = _fused(h, x, ws, bs, d)
    (hg, xg), wg, bg = _to((h, x), "cuda:0", torch.float32), _to(ws, "cuda:0", torch.float32), _to(bs, "cuda:0", torch.float32)
    e_torch = norm_rel(_chain(hg, xg, wg, bg, d).cpu().numpy(), ref)
    e = norm_rel(got, ref)
    print(f"gru half step B={B} {H}x{W} C={HID + inp} dir={d}: fused {e:.2e}, torch fp32 chain {e_torch:.2e}")
    assert np.isfinite(got).all()
    assert e <= REL_TOL


@pytest.mark.gpu
def test_direction_and_tap_order():
    ws, bs = _weights(320, "1")
    h, x = _inputs(21, 1, 320, 6, 7)
    out = [_fused(h, x, ws, bs, d) for d in (0, 1)]
    for d in (0, 1):
        assert norm_rel(out[d], _ref64(h, x, ws, bs, d)) <= REL_TOL
    assert norm_rel(out[0], out[1]) > 100 * REL_TOL
    flipped = tuple(np.ascontiguousarray(w[:, :, ::-1]) for w in ws)
    for d in (0, 1):
        assert norm_rel(_fused(h, x, flipped, bs, d), out[d]) > 100 * REL_TOL


@pytest.mark.gpu
def test_matches_reference_golden():
    from eraft_amd.gru import sepconv_gru
    g = load("gru_reference")
    for k, (seed, B, hidden, inp, H, W) in enumerate(g["cases"].tolist()):
        assert hidden == HID
        m = _module(inp, "cuda:0")
        h, x = _inputs(seed, B, inp, H, W)
        with torch.no_grad():
            out = sepconv_gru(m, torch.from_numpy(h).cuda(), torch.from_numpy(x).cuda()).cpu().numpy()
        e = norm_rel(out, g[f"h_out{k}"])
        print(f"gru golden {B}x{HID + inp}x{H}x{W}: {e:.2e}")
        assert e <= REL_TOL


@pytest.mark.gpu
def test_deterministic_and_capturable():
    from eraft_amd.gru import sepconv_gru
    m = _module(320, "cuda:0")
    h, x = (torch.from_numpy(a).cuda() for a in _inputs(31, 2, 320, 7, 9))
    with torch.no_grad():
        a = sepconv_gru(m, h, x)  # also the warm-up: the packs are made here, outside the capture
        b = sepconv_gru(m, h, x)
        assert bit_equal(a.cpu().numpy(), b.cpu().numpy())
        torch.cuda.synchronize()
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            c = sepconv_gru(m, h, x)
        gph.replay()
        torch.cuda.synchronize()
        assert bit_equal(a.cpu().numpy(), c.cpu().numpy())


@pytest.mark.gpu
def test_repack_follows_the_weights():
    from eraft_amd.gru import sepconv_gru
    h, x = _inputs(33, 1, 320, 6, 7)
    hg, xg = torch.from_numpy(h).cuda(), torch.from_numpy(x).cuda()
    m = _module(320, "cuda:0")
    with torch.no_grad():
        before = sepconv_gru(m, hg, xg).cpu().numpy()
        neww = prng.param_init("another.weight", tuple(m.convq2.weight.shape))
        m.convq2.weight.copy_(torch.from_numpy(neww))
        after = sepconv_gru(m, hg, xg).cpu().numpy()
    assert norm_rel(after, before) > 100 * REL_TOL
    assert norm_rel(after, _module64(m, h, x)) <= REL_TOL
    # a fresh module (new tensors, very likely in the freed storage) never sees the old packs
    del m
    gc.collect()
    m2 = _module(320, "cuda:0")
    with torch.no_grad():
        fresh = sepconv_gru(m2, hg, xg).cpu().numpy()
    assert norm_rel(fresh, _module64(m2, h, x)) <= REL_TOL
    assert norm_rel(fresh, before) <= REL_TOL  # the same prng weights as the first module's


@pytest.mark.gpu
def test_module_switch(monkeypatch):
    from eraft_amd.model import SepConvGRU
    m = _module(320, "cuda:0")
    h, x = (torch.from_numpy(a).cuda() for a in _inputs(35, 2, 320, 7, 9))
    with torch.no_grad():
        monkeypatch.setattr(SepConvGRU, "fused", False)
        plain = m(h, x)
        monkeypatch.setattr(SepConvGRU, "fused", True)
        fused = m(h, x)
    assert not bit_equal(plain.cpu().numpy(), fused.cpu().numpy())  # the fused kernels did run
    assert norm_rel(fused.cpu().numpy(), plain.cpu().numpy()) <= REL_TOL
    # autograd recording: the torch path, untouched
    hr = h.clone().requires_grad_(True)
    out_f = m(hr, x)
    monkeypatch.setattr(SepConvGRU, "fused", False)
    out_p = m(hr, x)
    assert out_f.grad_fn is not None
    assert bit_equal(out_f.detach().cpu().numpy(), out_p.detach().cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_conv", [True, False])
def test_e2e_with_fused_gru_matches_reference(monkeypatch, fuse_conv):
    """The g_e2e_dsec golden, cold and warm start, with the GRU on the fused kernels."""
    from eraft_amd.model import ERAFT, SepConvGRU
    from test_e2e import EPE_TOL, _epe, _model
    monkeypatch.setattr(SepConvGRU, "fused", True)
    monkeypatch.setattr(ERAFT, "fuse_lookup_conv", fuse_conv)
    g = load("g_e2e_dsec")
    seed, H, W, bins, iters = (int(v) for v in g["meta"])
    dev = "cuda:0"
    im1 = torch.from_numpy(prng.voxel_grid(seed, (1, bins, H, W))).to(dev)
    im2 = torch.from_numpy(prng.voxel_grid(seed + 2, (1, bins, H, W))).to(dev)
    model = _model(bins).to(dev)
    finit = torch.from_numpy(g["flow_init"]).to(dev)
    with torch.no_grad():
        low, ups = model(im1, im2, iters=iters)
        low_w, ups_w = model(im1, im2, iters=iters, flow_init=finit)
    errs = (_epe(low.cpu().numpy(), g["low"]), _epe(ups[-1][..., ::4, ::4].cpu().numpy(), g["up_sub"]),
            _epe(low_w.cpu().numpy(), g["low_warm"]), _epe(ups_w[-1][..., ::4, ::4].cpu().numpy(), g["up_warm_sub"]))
    print(f"e2e fused GRU (fuse_lookup_conv={fuse_conv}): cold low/up {errs[0]:.2e}/{errs[1]:.2e}, "
          f"warm low/up {errs[2]:.2e}/{errs[3]:.2e} px")
    assert all(e <= EPE_TOL for e in errs)
