"""Generate the golden fixtures in tests/golden/*.npz FROM THE REFERENCE ITSELF.

Run in the survey container only (needs /root/reference, never present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py

It imports the reference's own CorrBlock (model/corr.py:12-60) and coords_grid
(model/utils.py:24-27), feeds it inputs from tests/golden/prng.py (portable; only seeds are
stored) and records its outputs.  The fixtures are data (inputs' seeds + reference outputs),
never reference source.  Backward goldens come from the reference under torch autograd.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prng  # noqa: E402

REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")
from model.corr import CorrBlock  # noqa: E402  (reference)

torch.set_num_threads(8)


def fmaps(seed, B, D, H, W):
    return prng.gauss(seed, (B, D, H, W)), prng.gauss(seed + 1, (B, D, H, W))


def ref_build(f1, f2, L, r):
    return CorrBlock(torch.from_numpy(f1), torch.from_numpy(f2), num_levels=L, radius=r)


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"{name}: {os.path.getsize(path) / 1e6:.2f} MB")


def case_build_lookup(name, seed, B, D, H, W, L, r, sigmas, store_pyramid=True):
    f1, f2 = fmaps(seed, B, D, H, W)
    cb = ref_build(f1, f2, L, r)
    out = {"meta": np.array([seed, B, D, H, W, L, r], np.int64),
           "sigmas": np.array(sigmas, np.float32)}
    if store_pyramid:
        for l, p in enumerate(cb.corr_pyramid):
            out[f"pyr{l}"] = p.numpy()
    corr6 = CorrBlock.corr(torch.from_numpy(f1), torch.from_numpy(f2))
    out["corr_shape"] = np.array(corr6.shape, np.int64)
    for k, s in enumerate(sigmas):
        c = prng.lookup_coords(seed + 100 + k, B, H, W, s)
        out[f"coords{k}"] = c
        out[f"look{k}"] = cb(torch.from_numpy(c)).numpy()
    c = prng.special_coords(B, H, W)
    out["coords_special"] = c
    out["look_special"] = cb(torch.from_numpy(c)).numpy()
    save(name, **out)


def case_backward(name, seed, B, D, H, W, L, r, iters):
    f1, f2 = fmaps(seed, B, D, H, W)
    t1 = torch.from_numpy(f1).requires_grad_(True)
    t2 = torch.from_numpy(f2).requires_grad_(True)
    cb = CorrBlock(t1, t2, num_levels=L, radius=r)
    K = (2 * r + 1) ** 2
    loss = 0.0
    for t in range(iters):
        c = prng.lookup_coords(seed + 200 + t, B, H, W, 2.0 + t)
        g = prng.gauss(seed + 300 + t, (B, L * K, H, W))
        o = cb(torch.from_numpy(c))
        loss = loss + (o * torch.from_numpy(g)).sum()
    loss.backward()
    save(name, meta=np.array([seed, B, D, H, W, L, r, iters], np.int64),
         df1=t1.grad.numpy(), df2=t2.grad.numpy())


def case_dsec_spot(name, seed):
    """DSEC shape (B=1, 60x80, D=256): slices + fp64 checksums only (full pyramid is 122 MB)."""
    B, D, H, W, L, r = 1, 256, 60, 80, 4, 4
    f1, f2 = fmaps(seed, B, D, H, W)
    cb = ref_build(f1, f2, L, r)
    q = np.array([0, 1, 79, 80, 2399, 2400, 4719, 4799, 1234, 3000, 4321, 17, 555, 2048, 3333, 4000])
    out = {"meta": np.array([seed, B, D, H, W, L, r], np.int64), "q": q}
    for l, p in enumerate(cb.corr_pyramid):
        p = p.numpy()
        out[f"pyr{l}_rows"] = p[q]
        out[f"pyr{l}_sum"] = np.array([p.astype(np.float64).sum(), np.abs(p).astype(np.float64).sum()])
    c = prng.lookup_coords(seed + 100, B, H, W, 8.0)
    o = cb(torch.from_numpy(c)).numpy()
    out["look_q"] = o.reshape(B, -1, H * W)[:, :, q]
    out["look_sum"] = np.array([o.astype(np.float64).sum(), np.abs(o).astype(np.float64).sum()])
    save(name, **out)


def init_model(model):
    sd = model.state_dict()
    with torch.no_grad():
        for name, t in sd.items():
            v = prng.param_init(name, tuple(t.shape))
            if v is not None:
                t.copy_(torch.from_numpy(v))


def case_e2e(name, seed, H=480, W=640, bins=15, iters=12):
    """Full reference E-RAFT forward (model/eraft.py:89-146), random weights from
    prng.param_init, cold call then warm-start call with the reference's own forward splat
    (utils/image_utils.py:52-83, test.py:209).  flow_up is stored every 4th pixel."""
    from model.eraft import ERAFT
    from utils.image_utils import forward_interpolate_pytorch
    model = ERAFT({"subtype": "warm_start"}, n_first_channels=bins).eval()
    init_model(model)
    im1 = torch.from_numpy(prng.voxel_grid(seed, (1, bins, H, W)))
    im2 = torch.from_numpy(prng.voxel_grid(seed + 2, (1, bins, H, W)))
    with torch.no_grad():
        low, ups = model(im1, im2, iters=iters)
        finit = forward_interpolate_pytorch(low)
        model2 = ERAFT({"subtype": "warm_start"}, n_first_channels=bins).eval()
        init_model(model2)
        low_w, ups_w = model2(im1, im2, iters=iters, flow_init=finit)
    keys = [f"{k}:{tuple(v.shape)}" for k, v in model.state_dict().items()]
    save(name, meta=np.array([seed, H, W, bins, iters], np.int64), state_keys=np.array(keys),
         low=low.numpy(), up_sub=ups[-1][..., ::4, ::4].numpy(),
         up_mean_abs=np.array([ups[-1].abs().mean().item()]),
         flow_init=finit.numpy(), low_warm=low_w.numpy(), up_warm_sub=ups_w[-1][..., ::4, ::4].numpy())


def case_splat(name, seed):
    """Warm-start forward splat (utils/image_utils.py:10-83, forward_interpolate_pytorch):
    flows with fractional, exactly-integer (floor == ceil: the reference counts that corner
    twice), out-of-bounds and colliding targets; B = 2 at 17 x 23 and B = 1 at 60 x 80."""
    from utils.image_utils import forward_interpolate_pytorch
    out = {}
    cases = [("a", 2, 17, 23, 3.0), ("b", 1, 60, 80, 6.0)]
    for tag, B, H, W, sig in cases:
        f = prng.gauss(seed, (B, 2, H, W), sig)
        f[:, :, ::4, ::3] = np.round(f[:, :, ::4, ::3])          # integer displacements
        f[0, 0, 1, :5] = [40.0, -40.0, 0.0, -0.5, 1e4]           # far out / exact / half
        f[0, 1, 2, :4] = [0.0, 0.0, -3.0, 2.5]
        f[0, :, 3, :6] = 0.0                                     # several sources, one target
        out[f"flow_{tag}"] = f
        out[f"splat_{tag}"] = forward_interpolate_pytorch(torch.from_numpy(f)).numpy()
        seed += 1
    save(name, **out)


def case_voxel(name, seed):
    """DSEC event -> voxel grid (utils/dsec_utils.py:19-64 VoxelGrid.convert, normalize=True
    and False) on events shaped as loader_dsec.py:245-257 makes them: float32 rectified x, y
    (fractional, some out of the frame), t normalised to [0, 1], p in {0, 1}; repeated pixels
    collide.  Inputs from prng; outputs from the reference, run single-threaded as its own
    entry point pins it (main.py:2-5): put_(accumulate=True) on CPU is chunked over threads,
    so its summation order (and the low bits) depend on the thread count; one thread = the
    sequential event order."""
    from utils.dsec_utils import VoxelGrid
    torch.set_num_threads(1)
    out = {}
    for tag, M, C, H, W in (("a", 3000, 5, 12, 16), ("b", 40000, 15, 48, 64)):
        u = prng.uniform(seed, (4, M))
        x = (u[0] * (W + 2) - 1.0).astype(np.float32)
        y = (u[1] * (H + 2) - 1.0).astype(np.float32)
        x[::7] = np.floor(x[::7])                       # integer coordinates
        t = np.sort(u[2]).astype(np.float32)
        t = (t - t[0]) / (t[-1] - t[0])
        p = (u[3] > 0.5).astype(np.float32)
        ev = {k: torch.from_numpy(v.copy()) for k, v in (("x", x), ("y", y), ("t", t), ("p", p))}
        out[f"ev_{tag}"] = np.stack([x, y, t, p])
        out[f"meta_{tag}"] = np.array([M, C, H, W], np.int64)
        out[f"raw_{tag}"] = VoxelGrid((C, H, W), normalize=False).convert(ev).numpy()
        out[f"norm_{tag}"] = VoxelGrid((C, H, W), normalize=True).convert(ev).numpy()
        seed += 1
    save(name, **out)


def case_voxel_mvsec(name, seed):
    """MVSEC event -> voxel grid (utils/transformers.py:18-126 EventSequenceToVoxelGrid_Pytorch,
    the representation of loader/loader_mvsec_flow.py:35), normalize=True and False.  Events
    as the MVSEC loader holds them: [M, 4] float64 rows (t, x, y, p) with integer pixel
    coordinates, t ascending relative microsecond stamps, p in {0, 1}; duplicated stamps, the
    first/last bins and colliding pixels are included, and case "c" has all stamps equal
    (deltaT = 0 -> 1).  index_add_ on CPU adds sequentially in index order, so the thread
    count does not matter; run single-threaded anyway as main.py:2-5 does."""
    import types
    from utils.transformers import EventSequenceToVoxelGrid_Pytorch
    torch.set_num_threads(1)
    out = {}
    for tag, M, C, H, W in (("a", 3000, 5, 12, 16), ("b", 60000, 15, 260, 346), ("c", 500, 3, 8, 8)):
        u = prng.uniform(seed, (4, M)).astype(np.float64)
        x = np.floor(u[0] * W)
        y = np.floor(u[1] * H)
        t = np.sort(u[2] * 50000.0)          # relative microseconds (loader_mvsec_flow.py:170-172)
        t[::5] = np.floor(t[::5])             # some integer stamps
        t[10:20] = t[10]                      # repeated stamps
        if tag == "c":
            t[:] = 12345.0
        p = (u[3] > 0.5).astype(np.float64)
        ev = np.ascontiguousarray(np.stack([t, x, y, p], axis=1))
        seq = types.SimpleNamespace(features=ev, image_width=W, image_height=H)
        out[f"ev_{tag}"] = ev
        out[f"meta_{tag}"] = np.array([M, C, H, W], np.int64)
        for norm, key in ((False, "raw"), (True, "norm")):
            conv = EventSequenceToVoxelGrid_Pytorch(C, gpu=False, normalize=norm, forkserver=False)
            out[f"{key}_{tag}"] = conv(seq).numpy()
        seed += 1
    save(name, **out)


def voxel_edge_events():
    """The inputs of case_voxel_edges: {name: (ev [4, M] float32 rows x, y, t, p, (C, H, W))}
    for VoxelGrid and {name: (ev [M, 4] float64 rows t, x, y, p, (C, H, W))} for
    EventSequenceToVoxelGrid_Pytorch.  Written out by hand: every value is the point."""
    C, H, W = 5, 6, 8
    nan, inf = np.nan, np.inf
    d, m = {}, {}

    def dsec(name, rows):
        d[name] = (np.ascontiguousarray(np.array(rows, np.float32).T), (C, H, W))

    def mvsec(name, rows):
        m[name] = (np.ascontiguousarray(np.array(rows, np.float64)), (C, H, W))

    # degenerate windows: t[M-1] == t[0] -> t_n = 0/0 (or x/0) for every event -> Tensor.int()
    # gives INT_MIN -> no corner passes the mask -> the grid stays zero
    dsec("single", [(2.5, 3.25, 0.0, 1)])
    dsec("single_nan_t", [(2.5, 3.25, nan, 1)])            # what loader_dsec.py:246-247 hands over
    dsec("equal_stamps", [(2.5, 3.25, 0.5, 1), (1.0, 2.0, 0.5, 0), (6.75, 0.5, 0.5, 1), (2.5, 3.25, 0.5, 0)])
    dsec("ends_equal", [(2.5, 3.25, 0.0, 1), (1.0, 2.0, 0.5, 0), (6.75, 0.5, 0.25, 1), (2.5, 3.25, 0.0, 0)])
    dsec("ends_equal_neg", [(2.5, 3.25, 0.5, 1), (1.0, 2.0, 0.75, 0), (6.75, 0.5, 0.25, 1), (2.5, 3.25, 0.5, 0)])

    # NaN / inf / beyond-int32 coordinates between ordinary events that vote into cells (0, 0),
    # (0, 1), (1, 0), (1, 1) of bin 0: an admitted event would change a sum or its order
    big = 2147483520.0                                      # the largest float32 below 2^31
    odd = [(nan, 0.5), (0.25, nan), (nan, nan), (inf, 0.5), (-inf, 0.5), (3e9, 0.5), (-3e9, 0.5), (big, 0.5),
           (0.25, inf), (0.25, -inf), (0.25, 3e9), (0.25, -3e9), (0.25, big), (-big, 0.5), (0.25, -big)]
    rows = []
    for k, (ox, oy) in enumerate(odd):
        rows.append((0.125 + 0.0625 * (k % 7), 0.875 - 0.09375 * (k % 5), 0.0, k % 3 != 0))
        rows.append((ox, oy, 0.0, k % 2))
    rows.append((0.3125, 0.4375, 0.0, 1))
    rows.append((5.5, 4.5, 0.0, 1))                         # the last stamp: t_n = C - 1
    ts = np.concatenate([np.arange(len(rows) - 1) * np.float32(1 / 128), [1.0]])  # ascending, bin 0 but the last
    dsec("nan_coords", [(x, y, t, p) for (x, y, _, p), t in zip(rows, ts)])

    dsec("outside", [
        (-0.5, -0.25, 0.0, 1),       # trunc toward zero: corner (0, 0), negative weights on column / row 1
        (0.5, 0.25, 0.125, 0),
        (-1.5, 2.5, 0.25, 1),        # corner -1 dropped, corner 0 weighs -0.5
        (W - 0.5, 2.25, 0.375, 1),   # corner W dropped
        (float(W), 1.5, 0.5, 0),     # both corners out
        (3.5, H - 0.5, 0.625, 1),
        (2.5, float(H), 0.75, 0),
        (-1.0, 3.0, 0.8125, 1),      # corner 0 with weight exactly 0
        (0.5, 2.5, 0.875, 1),
        (7.25, 5.5, 1.0, 0)])

    # unsorted stamps: t[0] = 2, t[M-1] = 6, span 4 = C - 1, so t_n = t - 2
    dsec("t_outside", [
        (2.5, 3.25, 2.0, 1),         # t_n 0
        (2.5, 3.25, 1.5, 0),         # -0.5: truncates to bin 0, weight 0.5
        (2.5, 3.25, 0.5, 1),         # -1.5: bin -1, dropped
        (2.5, 3.25, 6.5, 1),         # C - 0.5: bin C - 1, weight 0.5
        (2.5, 3.25, 9.0, 0),         # C + 2: dropped
        (1.75, 4.5, 3.25, 0),        # 1.25
        (2.5, 3.25, 6.0, 1)])        # exactly C - 1, weight 1

    polarity = [(1.5, 2.5, 0.0, 0), (1.5, 2.5, 0.125, 1), (1.25, 2.75, 0.25, 0.5), (4.5, 1.5, 0.5, 2),
                (4.25, 1.25, 0.5625, -1), (6.5, 4.5, 0.75, nan),   # a pixel no other event touches
                (1.5, 2.5, 1.0, 1)]
    dsec("polarity", polarity)
    dsec("nan_cell", polarity)                              # the same events, read for the normalised grid

    # normalisation rules: integer coordinates, stamps on exact bins -> every vote is +-1 (or +-0)
    dsec("one_cell", [(2, 3, 0.0, 1), (-5, 0, 1.0, 1)])    # std of one value is NaN -> v - mean = 0
    dsec("equal_cells", [(2, 3, 0.0, 1), (5, 1, 1.0, 1)])  # std 0 -> v - mean = 0
    dsec("cancelled", [(1, 1, 0.0, 1), (1, 1, 0.0, 1), (6, 4, 0.25, 1), (5, 5, 0.75, 1), (5, 5, 0.75, 0),
                       (3, 2, 1.0, 0)])                     # {+2, +1, -1} and a cell that cancels to 0

    mvsec("wrap", [
        (0.0, 1, 1, 1), (50.0, W + 2, 2, 1),    # x = W + 2 at row 2: two cells into row 3
        (100.0, 2, 3, 0), (150.0, -1, 3, 1),    # x = -1 at row 3: the last cell of row 2
        (200.0, 7, 2, 1), (250.0, -0.5, 4, 0),  # x = -0.5 truncates to 0
        (300.0, 0, 4, 1), (400.0, 3, 5, 1)])
    mvsec("nan_t", [(0.0, 1, 1, 1), (120.0, 2, 3, 0), (nan, 2, 3, 1), (260.0, 2, 3, 1), (400.0, 3, 5, 0)])
    mvsec("one_cell", [(100.0, 2, 3, 1), (100.0, 2, 3, 1)])
    mvsec("equal_cells", [(0.0, 2, 3, 1), (400.0, 5, 1, 1)])
    mvsec("cancelled", [(0.0, 1, 1, 1), (0.0, 1, 1, 1), (100.0, 6, 4, 1), (300.0, 5, 5, 1), (300.0, 5, 5, 0),
                        (400.0, 3, 2, 0)])
    return d, m


def case_voxel_edges(name):
    """Both voxel representations at the edges the bulk fixtures leave out: degenerate time
    windows, NaN / inf / beyond-int32 coordinates, corners and bins just outside the grid, odd
    polarities, MVSEC events whose flat index wraps into a neighbouring row, and grids on which
    each branch of the normalisation is the whole answer.  Only events the reference accepts."""
    import types
    from utils.dsec_utils import VoxelGrid
    from utils.transformers import EventSequenceToVoxelGrid_Pytorch
    torch.set_num_threads(1)
    d, m = voxel_edge_events()
    out = {}
    for tag, (ev, (C, H, W)) in d.items():
        evt = {k: torch.from_numpy(ev[i].copy()) for i, k in enumerate("xytp")}
        out[f"d_ev_{tag}"] = ev
        out[f"d_meta_{tag}"] = np.array([ev.shape[1], C, H, W], np.int64)
        out[f"d_raw_{tag}"] = VoxelGrid((C, H, W), normalize=False).convert(evt).numpy()
        out[f"d_norm_{tag}"] = VoxelGrid((C, H, W), normalize=True).convert(evt).numpy()
    # observed with Tensor.int() on an x86 CPU (NaN, +-inf -> INT_MIN): if a torch build converts
    # differently these grids are not zero, and the fixture must not be made silently
    for tag in ("single", "single_nan_t", "equal_stamps", "ends_equal", "ends_equal_neg"):
        assert not out[f"d_raw_{tag}"].any() and not out[f"d_norm_{tag}"].any(), tag
    for tag, (ev, (C, H, W)) in m.items():
        seq = types.SimpleNamespace(features=ev, image_width=W, image_height=H)
        out[f"m_ev_{tag}"] = ev
        out[f"m_meta_{tag}"] = np.array([ev.shape[0], C, H, W], np.int64)
        for norm, key in ((False, "raw"), (True, "norm")):
            conv = EventSequenceToVoxelGrid_Pytorch(C, gpu=False, normalize=norm, forkserver=False)
            out[f"m_{key}_{tag}"] = conv(seq).numpy()
    save(name, **out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "voxel_edges":
        case_voxel_edges("g_voxel_edges")
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "voxel_mvsec":
        case_voxel_mvsec("g_voxel_mvsec", 51)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "voxel":
        case_voxel("g_voxel", 41)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "splat":
        case_splat("g_splat", 31)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "e2e":
        case_e2e("g_e2e_dsec", 21)
        sys.exit(0)
    case_build_lookup("g_b1_d32_16x16", 11, 1, 32, 16, 16, 4, 4, [0.0, 3.0, 20.0])
    case_build_lookup("g_b2_d256_17x23", 12, 2, 256, 17, 23, 4, 4, [8.0])
    case_build_lookup("g_b2_d64_16x20_L2r3", 13, 2, 64, 16, 20, 2, 3, [5.0])
    case_build_lookup("g_degenerate_b1_d32_12x16", 14, 1, 32, 12, 16, 4, 4, [3.0])
    case_build_lookup("g_degenerate_b1_d16_15x21", 15, 1, 16, 15, 21, 4, 4, [3.0])
    case_backward("g_bwd_b2_d16_18x24", 16, 2, 16, 18, 24, 4, 4, 12)
    case_backward("g_bwd_b1_d32_17x23_L2r3", 17, 1, 32, 17, 23, 2, 3, 3)
    case_dsec_spot("g_dsec_spot", 18)
