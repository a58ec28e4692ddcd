"""GPU suite for the point-cloud renderer: ops.render_points (csrc/render.hip) bit for bit against tests/render_law.py over
every size at which tiling can go wrong and under every tile size, lattices aimed at the tile and image borders, contended
and degenerate inputs, the output buffers — and the PNGs core/experiments.py writes with save_plots=True, each against the
law's rendering of the array saved beside it, with everything else unchanged by the drawing."""
import copy
import os

import numpy as np
import pytest
import torch

import render_law
from conftest import fixture_state_, golden

pytestmark = pytest.mark.gpu

CUDA = "cuda"
IDENTITY = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]], np.float32)    # u = x, v = y, w = z
PALETTE = [(31, 119, 180), (214, 39, 40), (250, 250, 5), (0, 0, 0), (255, 255, 255), (1, 2, 3), (99, 98, 97), (128, 127, 126)]
BACKGROUND = (250, 240, 230)


class tile:
    """hp_render_points_set_tile(side) for the length of a block; 0 = the launcher's choice."""

    def __init__(self, side):
        self.side = side

    def __enter__(self):
        from hyperpocket_amd import ops
        self.before = ops.load_library().hp_render_points_set_tile(self.side)
        assert self.before >= 0

    def __exit__(self, *exc):
        from hyperpocket_amd import ops
        ops.load_library().hp_render_points_set_tile(self.before)


def _views(V, size):
    from hyperpocket_amd.utils.render import view_matrix
    return np.stack([view_matrix(e, a, size) for e, a in ((10, 240), (65, 20), (-30, 135))[:V]])


def _layers(n, L):
    """L = 3: the middle layer is empty."""
    return [n] if L == 1 else [n // 3, n // 3, n]


def _gpu(points, views, ends, palette, radius2, size, fog, background=BACKGROUND, **kw):
    from hyperpocket_amd import ops
    out = ops.render_points(torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(CUDA), ends, palette, radius2,
                            torch.from_numpy(np.ascontiguousarray(views, np.float32)).to(CUDA), size, fog=fog,
                            background=background, ids=True, **kw)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def _check(points, views, ends, palette, radius2, size, fog, sides=(0,)):
    want = render_law.render_batch(points, views, ends, palette, radius2, size, fog, BACKGROUND)
    for side in sides:
        with tile(side):
            image, ids = _gpu(points, views, ends, palette, radius2, size, fog)
        assert image.shape == want[0].shape and ids.shape == want[1].shape
        assert np.array_equal(ids, want[1]), (side, int((ids != want[1]).sum()))
        assert np.array_equal(image, want[0]), (side, int((image != want[0]).sum()))
    return want


# (B, n, V, L, radius2 per layer, (W, H), tile side): every value of the issue's lists at least once, every size under the
# launcher's own tile and under a smaller and a larger one
CASES = [
    (1, 1, 1, 1, [0], (1, 1), 0),
    (1, 63, 1, 1, [1], (1, 1), 8),
    (1, 64, 1, 1, [64], (1, 1), 128),
    (3, 64, 3, 3, [0, 1, 2], (37, 53), 0),
    (1, 65, 1, 1, [4], (37, 53), 16),
    (1, 1000, 1, 3, [2, 9, 64], (37, 53), 8),
    (1, 65, 1, 3, [9, 1, 0], (37, 53), 32),
    (1, 1000, 1, 1, [2], (128, 128), 0),
    (3, 65, 1, 1, [9], (128, 128), 128),
    (1, 1000, 3, 3, [1, 4, 64], (128, 128), 64),
    (3, 63, 3, 1, [2], (128, 128), 16),
    (1, 1000, 1, 3, [0, 2, 9], (129, 130), 0),
    (1, 1000, 1, 1, [64], (129, 130), 128),
    (1, 63, 1, 1, [64], (129, 130), 64),
    (3, 1000, 1, 1, [1], (129, 130), 32),
    (1, 1, 1, 3, [0, 0, 64], (129, 130), 0),
    (1, 1000, 1, 1, [4], (129, 130), 8),
    (1, 1000, 1, 3, [2, 2, 9], (500, 500), 0),
    (1, 1000, 1, 1, [64], (500, 500), 128),
    (1, 64, 3, 1, [4], (500, 500), 64),
    (1, 1000, 1, 1, [0], (500, 500), 8),
    (1, 65, 1, 3, [1, 9, 2], (500, 500), 32),
    (3, 1, 1, 1, [9], (500, 500), 0),
    (1, 1000, 1, 1, [9], (500, 500), 16),
]


@pytest.mark.parametrize("B,n,V,L,radius2,size,side", CASES,
                         ids=[f"B{c[0]}-n{c[1]}-V{c[2]}-L{c[3]}-r{'.'.join(map(str, c[4]))}-{c[5][0]}x{c[5][1]}-t{c[6]}" for c in CASES])
def test_image_and_ids_equal_the_law(B, n, V, L, radius2, size, side):
    """Clouds somewhat larger than the cube the view frames, so that some points leave the image on every side; the first
    point of each stays near the centre."""
    rng = np.random.RandomState(1000 * n + 10 * size[0] + B + V)
    points = ((rng.rand(B, n, 3) - 0.5) * 1.9).astype(np.float32)
    points[:, 0] *= np.float32(0.125)
    want = _check(points, _views(V, size), _layers(n, L), PALETTE[:L], radius2, size, fog=200, sides=(side,))
    assert (want[1] >= 0).any()


def test_lattice_on_the_tile_and_image_borders():
    """Points at integer coordinates — exactly on pixel boundaries — at every tile edge of the plan and at the image's own
    edges, offset by -r-1, -r, -1, 0, 1 and r in both axes: a splat that crosses a border must be whole on both sides."""
    from hyperpocket_amd import ops
    size = (150, 140)
    for side in (0, 16):
        with tile(side):
            plan = ops.render_points_plan(1, 1, size)
        assert plan.tiles_x >= 2 and plan.tiles_y >= 2
        for radius2 in (1, 9, 64):
            r = int(np.sqrt(radius2))
            offsets = sorted({-r - 1, -r, -1, 0, 1, r})
            xs = sorted({e + o for e in list(range(0, size[0], plan.tile_w))[:4] + [size[0]] for o in offsets})
            ys = sorted({e + o for e in list(range(0, size[1], plan.tile_h))[:4] + [size[1]] for o in offsets})
            pts = np.array([(x, y, 0) for y in ys for x in xs], np.float32)
            pts[:, 2] = ((np.arange(len(pts)) * 37) % 101) / 128.0          # depths that interleave along rows and columns
            want = _check(pts[None], IDENTITY, [len(pts)], PALETTE[:1], [radius2], size, fog=255, sides=(side,))
            assert (want[1][0, 0, :, plan.tile_w - 1] >= 0).any() and (want[1][0, 0, :, plan.tile_w] >= 0).any()
            assert (want[1][0, 0, plan.tile_h - 1] >= 0).any() and (want[1][0, 0, plan.tile_h] >= 0).any()


def test_identical_points_contend_for_one_neighbourhood():
    pts = np.tile(np.array([[17.5, 20.25, 0.3]], np.float32), (2048, 1))
    want = _check(pts[None], IDENTITY, [2048], PALETTE[:1], [9], (37, 53), fog=96, sides=(0, 8))
    assert set(np.unique(want[1]).tolist()) == {-1, 0} and (want[1] == 0).sum() == 29


def test_bad_and_out_of_range_inputs():
    W, H = 40, 30
    eps = np.float32(2.0 ** -26)
    rows = [(5.5, 5.5, 0.125 + eps), (5.5, 5.5, 0.125),              # equal zq, different w: the lower index wins
            (np.nan, 3, 0.5), (3, np.nan, 0.5), (3, 3, np.nan), (np.inf, 3, 0.5), (3, -np.inf, 0.5), (3, 3, np.inf),
            (3, 3, -np.inf), (1e30, 3, 0.5), (3, -1e30, 0.5), (12, 3, 1e30), (3e9, 3, 0.5), (3, -3e9, 0.5), (14, 3, -3e9),
            (-7.5, 25, 0.5), (-9.0, 12, 0.5), (-9.5, 14, 0.5), (W + 7.5, 10, 0.5), (W + 8.99, 12, 0.5), (W + 9.0, 14, 0.5),
            (30, -7.5, 0.5), (22, -9.0, 0.5), (24, -9.5, 0.5), (20, H + 7.5, 0.5), (22, H + 8.99, 0.5), (24, H + 9.0, 0.5),
            (30.5, 20.5, 0.75)]
    pts = np.array(rows, np.float32)
    assert pts[0, 2] != pts[1, 2]
    want = _check(pts[None], IDENTITY, [len(pts)], PALETTE[:1], [64], (W, H), fog=255, sides=(0, 16))
    shown = set(np.unique(want[1]).tolist())
    # a 0 in the view times an infinite coordinate is NaN: rows with an infinity or a NaN anywhere are dropped; a huge finite
    # depth is clamped; of the rows outside an edge, those 7.5 pixels out reach it with the one pixel at the tip of their disc
    assert shown == {-1, 0, 11, 14, 15, 18, 21, 24, 27}
    # under a view that scales, 1e30 overflows on the way: inf - inf, NaN, dropped — the same in the law and on the device
    _check(pts[None] * np.float32(0.01), _views(1, (W, H)), [len(pts)], PALETTE[:1], [4], (W, H), fog=255)


def test_output_buffers_streams_and_repeatability():
    from hyperpocket_amd import ops
    rng = np.random.RandomState(7)
    size, ends, radius2 = (129, 130), [200, 300], [2, 9]
    pts = torch.from_numpy(((rng.rand(2, 300, 3) - 0.5) * 1.5).astype(np.float32)).to(CUDA)
    views = torch.from_numpy(_views(3, size)).to(CUDA)
    want = render_law.render_batch(pts.cpu().numpy(), views.cpu().numpy(), ends, PALETTE[:2], radius2, size, 96, BACKGROUND)
    image = torch.full((2, 3, 130, 129, 3), 0xAB, dtype=torch.uint8, device=CUDA)
    ids = torch.full((2, 3, 130, 129), 0xABABABAB - (1 << 32), dtype=torch.int32, device=CUDA)
    got = ops.render_points(pts, ends, PALETTE[:2], radius2, views, size, fog=96, background=BACKGROUND, out=(image, ids), ids=True)
    assert got[0] is image and got[1] is ids
    assert np.array_equal(image.cpu().numpy(), want[0]) and np.array_equal(ids.cpu().numpy(), want[1])
    alone = torch.full_like(image, 0xAB)
    assert ops.render_points(pts, ends, PALETTE[:2], radius2, views, size, fog=96, background=BACKGROUND, out=alone) is alone
    assert torch.equal(alone, image)                               # ids=None: the same image
    again = ops.render_points(pts, ends, PALETTE[:2], radius2, views, size, fog=96, background=BACKGROUND, ids=True)
    assert torch.equal(again[0], image) and torch.equal(again[1], ids)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        other = ops.render_points(pts, ends, PALETTE[:2], radius2, views, size, fog=96, background=BACKGROUND, ids=True)
    stream.synchronize()
    assert torch.equal(other[0], image) and torch.equal(other[1], ids)
    empty = ops.render_points(pts[:0], ends, PALETTE[:2], radius2, views, size)
    assert tuple(empty.shape) == (0, 3, 130, 129, 3) and empty.dtype == torch.uint8


def test_wrapper_refuses_what_the_library_would():
    from hyperpocket_amd import HipExtensionError, ops
    pts, views = torch.zeros(1, 4, 3, device=CUDA), torch.zeros(1, 3, 4, device=CUDA)
    for kw in (dict(layer_ends=[3]), dict(layer_ends=[3, 2, 4], palette=PALETTE[:3], radius2=[1, 1, 1]), dict(radius2=[65]),
               dict(size=(0, 4)), dict(size=(4, 4097)), dict(fog=256), dict(palette=[(1, 2, 256)]), dict(palette=PALETTE[:2]),
               dict(views=torch.zeros(1, 4, 3, device=CUDA)), dict(points=torch.zeros(1, 4, 3, device=CUDA).double())):
        args = dict(points=pts, layer_ends=[4], palette=PALETTE[:1], radius2=[1], views=views, size=(8, 8))
        args.update(kw)
        with pytest.raises(HipExtensionError):
            ops.render_points(**args)


def test_render_clouds_overlay_and_save_plot(tmp_path):
    from hyperpocket_amd.utils import render as R
    rng = np.random.RandomState(3)
    clouds, over = (rng.rand(2, 100, 3).astype(np.float32) - 0.5), (rng.rand(2, 7, 3).astype(np.float32) - 0.5)
    size = (64, 48)
    got = R.render_clouds(torch.from_numpy(clouds).to(CUDA), overlay=over, size=size)
    want = render_law.render_batch(np.concatenate([clouds, over], 1), R.view_matrix(size=size)[None], [100, 107], R.DEFAULT_PALETTE,
                                   [R.DEFAULT_RADIUS2, R.DEFAULT_OVERLAY_RADIUS2], size, R.DEFAULT_FOG, R.DEFAULT_BACKGROUND)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want[0])
    assert (want[1] >= 100).any()                                  # the overlay shows
    X = clouds[0].T.copy()                                         # (3, n), as the reference's save_plot takes it
    for k, x in enumerate((X, torch.from_numpy(X), torch.from_numpy(X).to(CUDA))):
        path = R.save_plot(x, 12, k, str(tmp_path), "gt")
        assert path == os.path.join(str(tmp_path), f"12_{k}_gt.png")
        assert np.array_equal(R.read_png(path), _default_rendering(clouds[0]))


_RENDERED = {}


def _default_rendering(cloud):
    """The law's image of one (n,3) cloud under utils/render.py's defaults, computed once per array."""
    from hyperpocket_amd.utils import render as R
    key = cloud.tobytes()
    if key not in _RENDERED:
        _RENDERED[key] = render_law.render(cloud, R.DEFAULT_VIEW, [len(cloud)], R.DEFAULT_PALETTE[:1], [R.DEFAULT_RADIUS2],
                                           R.DEFAULT_SIZE, R.DEFAULT_FOG, R.DEFAULT_BACKGROUND)[0]
    return _RENDERED[key]


# ------------------------------------------------------------------------------------------------
# the experiments' PNGs
# ------------------------------------------------------------------------------------------------
def trained_model():
    """The seeded-init model brought to model_trained.npz's operating point (completions of unit scale), in eval mode."""
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel
    cfg = {"random_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
           "real_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
           "hyper_network": {"use_bias": True, "relu_slope": 0.2},
           "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                              "layer_out_channels": [32, 64, 128, 64]},
           "target_network_input": {"constant": False, "normalization": {"enable": True, "type": "progressive", "epoch": 100}}}
    gm = golden("model_trained")
    torch.manual_seed(int(gm["seed"]))
    model = FullModel(copy.deepcopy(cfg))
    model.apply(weights_init)
    model = model.cuda()
    fixture_state_(model.state_dict(), gm)
    return model.eval(), gm


def _cloud(n, seed, stretch=(1.0, 0.4, 0.5)):
    r = np.random.RandomState(seed)
    return ((r.rand(n, 3) - 0.5) * np.asarray(stretch)).astype(np.float32)


def _run_twice(tmp_path_factory, experiment):
    """`experiment(model, results_dir, save_plots)` without and with plots, each on a fresh model from the same seeds ->
    per run {"dir", "files": name -> bytes, "result", "torch", "cuda", "numpy"}."""
    runs = {}
    for plots in (False, True):
        results_dir = tmp_path_factory.mktemp("plots" if plots else "plain")
        model, gm = trained_model()
        torch.manual_seed(31)
        torch.cuda.manual_seed(32)
        np.random.seed(33)
        result, sub = experiment(model, str(results_dir), int(gm["epoch"]), plots)
        d = results_dir / sub
        runs[plots] = {"dir": d, "files": {name: (d / name).read_bytes() for name in sorted(os.listdir(d))}, "result": result,
                       "torch": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(), "numpy": np.random.get_state()}
    return runs


def _assert_only_pngs_were_added(runs, want_pngs):
    plain, plots = runs[False], runs[True]
    assert not [name for name in plain["files"] if name.endswith(".png")]
    assert sorted(name for name in plots["files"] if name.endswith(".png")) == sorted(want_pngs)
    assert {k: v for k, v in plots["files"].items() if not k.endswith(".png")} == plain["files"]
    assert torch.equal(plots["torch"], plain["torch"]) and torch.equal(plots["cuda"], plain["cuda"])
    a, b = plots["numpy"], plain["numpy"]
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.fixture(scope="module")
def fixed_runs(tmp_path_factory):
    from hyperpocket_amd.core.experiments import fixed

    def experiment(model, results_dir, epoch, plots):
        items = [(_cloud(64, 60 + i), 0, 0, i) for i in range(2)]   # a map-style dataset of (existing, missing, gt, idx)
        return fixed(model, torch.device(CUDA), {"blob": items}, results_dir, epoch, std=0.2, noises_per_item=2, batch_size=2,
                     save_plots=plots), "fixed"
    return _run_twice(tmp_path_factory, experiment)


def test_fixed_plots_change_nothing_else(fixed_runs):
    _assert_only_pngs_were_added(fixed_runs, [f"blob_{i}_{j}_fixed_reconstructed.png" for i in range(2) for j in range(2)]
                                 + [f"blob_{i}_existing.png" for i in range(2)])
    (ex_a, gen_a), (ex_b, gen_b) = fixed_runs[False]["result"], fixed_runs[True]["result"]
    assert torch.equal(gen_a, gen_b) and len(ex_a) == len(ex_b) == 2 and all(torch.equal(a, b) for a, b in zip(ex_a, ex_b))


def test_fixed_plots_are_the_laws_rendering_of_the_arrays_beside_them(fixed_runs):
    from hyperpocket_amd.utils.render import read_png
    d = fixed_runs[True]["dir"]
    for i in range(2):
        assert np.array_equal(read_png(str(d / f"blob_{i}_existing.png")), _default_rendering(np.load(d / f"blob_{i}_existing.npy").T.copy()))
        for j in range(2):
            cloud = np.load(d / f"blob_{i}_{j}_reconstruction.npy").T.copy()
            assert np.array_equal(read_png(str(d / f"blob_{i}_{j}_fixed_reconstructed.png")), _default_rendering(cloud)), (i, j)


@pytest.fixture(scope="module")
def slice_runs(tmp_path_factory):
    from hyperpocket_amd.core.experiments import same_model_different_slices

    def experiment(model, results_dir, epoch, plots):
        dataset = {"car": [(None, None, _cloud(64, 100 + i), i) for i in range(3)]}
        return same_model_different_slices(model, torch.device(CUDA), dataset, results_dir, epoch, amount=1, slices_number=2,
                                           std=0.2, seed=9, save_plots=plots), "same_model_different_slices"
    return _run_twice(tmp_path_factory, experiment)


def test_slices_plots_change_nothing_else(slice_runs):
    _assert_only_pngs_were_added(slice_runs, ["car_0_gt.png"] + [f"car_0_{j}_{side}_rec.png" for j in range(2) for side in "fs"])
    assert torch.equal(slice_runs[False]["result"], slice_runs[True]["result"])


def test_slices_plots_are_the_laws_rendering_of_the_arrays_beside_them(slice_runs):
    from hyperpocket_amd.utils.render import read_png
    d = slice_runs[True]["dir"]
    assert np.array_equal(read_png(str(d / "car_0_gt.png")), _default_rendering(np.load(d / "car_0_gt.npy")))
    for j in range(2):
        for side in "fs":
            cloud = np.load(d / f"car_0_{j}_{side}_rec.npy").T.copy()
            assert np.array_equal(read_png(str(d / f"car_0_{j}_{side}_rec.png")), _default_rendering(cloud)), (j, side)
