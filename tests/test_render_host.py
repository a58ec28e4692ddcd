"""CPU suite for the renderer's host side: utils/render.py's view matrix, PNG writer and reader and contact sheet, and the
C ABI of csrc/render.hip as far as it goes without a GPU — every rejected argument and the plan query."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import render_law
from conftest import PKG_DIR


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return ctypes.CDLL(mod.build(verbose=False))


# ------------------------------------------------------------------------------------------------
# view_matrix
# ------------------------------------------------------------------------------------------------
VIEWS = [(10.0, 240.0, (500, 500)), (35.0, -60.0, (320, 200)), (0.0, 0.0, (64, 128)), (80.0, 123.0, (37, 53))]


@pytest.mark.parametrize("elev,azim,size", VIEWS)
def test_view_matrix_is_a_scaled_rotation_that_keeps_the_cube_on_screen(elev, azim, size):
    from hyperpocket_amd.utils.render import view_matrix
    M = view_matrix(elev, azim, size)
    assert M.dtype == np.float32 and M.shape == (3, 4)
    a, b, c = (M[k, :3].astype(np.float64) for k in range(3))
    scale = min(size) / 2 / (np.sqrt(3.0) / 2)
    # one float32 rounding per entry: 2^-24 relative each, 3 products per dot
    assert abs(a.dot(b)) <= 4 * 2.0 ** -24 * scale ** 2
    assert abs(np.linalg.norm(a) - np.linalg.norm(b)) <= 4 * 2.0 ** -24 * scale
    assert abs(np.linalg.norm(a) - scale) <= 4 * 2.0 ** -24 * scale
    assert abs(a.dot(c)) <= 1e-6 * scale and abs(b.dot(c)) <= 1e-6 * scale
    corners = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float32)
    u, v, w = render_law.project(corners, M)
    assert (u >= 0).all() and (u < size[0]).all() and (v >= 0).all() and (v < size[1]).all()
    assert (w >= 0).all() and (w < 1).all()
    centre = render_law.project(np.zeros((1, 3), np.float32), M)
    assert (centre[0][0], centre[1][0], centre[2][0]) == (size[0] / 2, size[1] / 2, 0.5)


def test_view_matrix_other_cube_and_extent():
    from hyperpocket_amd.utils.render import DEFAULT_SIZE, DEFAULT_VIEW, view_matrix
    assert np.array_equal(DEFAULT_VIEW, view_matrix(10, 240, DEFAULT_SIZE)) and DEFAULT_SIZE == (500, 500)
    M = view_matrix(20, 30, (100, 100), lo=0.0, hi=2.0)
    u, v, w = render_law.project(np.array([[1, 1, 1], [0, 0, 0], [2, 2, 2]], np.float32), M)
    assert abs(u[0] - 50) < 1e-4 and abs(v[0] - 50) < 1e-4 and abs(w[0] - 0.5) < 1e-6
    assert (u[1:] >= 0).all() and (u[1:] < 100).all() and (w[1:] >= 0).all() and (w[1:] < 1).all()
    # extent: the distance from the centre that reaches the edge of the shorter side
    M = view_matrix(0, 0, (200, 100), extent=0.25)                 # looking down -x: right is +y, up is +z
    u, v, w = render_law.project(np.array([[0, 0.25, 0], [0, 0, 0.25], [0.25, 0, 0]], np.float32), M)
    assert np.allclose([u[0], v[0]], [150, 50], atol=1e-4) and np.allclose([u[1], v[1]], [100, 0], atol=1e-4)
    assert abs(w[2]) < 1e-6                                        # the point nearest the eye


def test_screen_directions_of_the_world_axes_agree_with_matplotlib():
    """The reference's camera: elev 10, azim 240 (utils/pcutil.py).  M is rounded to float32 once, 6e-8 relative; 1e-6 on
    the unit screen directions leaves room to spare."""
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from mpl_toolkits.mplot3d import proj3d
    from hyperpocket_amd.utils.render import view_matrix
    fig = plt.figure(figsize=(5, 5))
    try:
        ax = fig.add_subplot(projection="3d")
        ax.view_init(elev=10, azim=240)
        ax.set_proj_type("ortho")
        ax.set_box_aspect((1, 1, 1))
        for set_lim in (ax.set_xlim, ax.set_ylim, ax.set_zlim):
            set_lim(-0.5, 0.5)
        P = ax.get_proj()
        origin = np.array(proj3d.proj_transform(0, 0, 0, P)[:2])
        M = view_matrix(10, 240, (500, 500)).astype(np.float64)
        for axis in range(3):
            e = np.zeros(3)
            e[axis] = 1
            theirs = np.array(proj3d.proj_transform(*e, P)[:2]) - origin
            ours = np.array([M[0, axis], -M[1, axis]])             # image rows grow downwards
            assert np.abs(theirs / np.linalg.norm(theirs) - ours / np.linalg.norm(ours)).max() <= 1e-6, axis
    finally:
        plt.close(fig)


# ------------------------------------------------------------------------------------------------
# PNG
# ------------------------------------------------------------------------------------------------
def _chunks(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + length]
        crc, = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        out.append((kind, body, crc))
        pos += 12 + length
    assert pos == len(data)
    return out


@pytest.mark.parametrize("W,H", [(1, 1), (37, 53), (500, 500)])
def test_png_round_trip(tmp_path, W, H):
    from hyperpocket_amd.utils.render import read_png, write_png
    a = np.random.RandomState(W).randint(0, 256, (H, W, 3)).astype(np.uint8)
    a[0, 0] = (0, 128, 255)
    for level in (1, 6):
        path = str(tmp_path / f"a{level}.png")
        assert write_png(path, a, level=level) == path
        assert np.array_equal(read_png(path), a)
        chunks = _chunks(path)
        assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        for kind, body, crc in chunks:
            assert zlib.crc32(kind + body) & 0xFFFFFFFF == crc, kind
        assert struct.unpack(">IIBBBBB", chunks[0][1]) == (W, H, 8, 2, 0, 0, 0)            # 8-bit RGB, not interlaced
        raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(H, 1 + 3 * W)
        assert not raw[:, 0].any()                                                         # filter type 0 on every row
    assert np.array_equal(read_png(write_png(str(tmp_path / "t.png"), torch.from_numpy(a))), a)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), a)


def test_png_refuses_what_it_does_not_handle(tmp_path):
    from hyperpocket_amd.utils.render import read_png, write_png
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            write_png(str(tmp_path / "bad.png"), bad)
    path = write_png(str(tmp_path / "ok.png"), np.full((3, 2, 3), 7, np.uint8))
    data = bytearray(open(path, "rb").read())
    data[-20] ^= 1                                                 # inside IDAT
    open(path, "wb").write(bytes(data))
    with pytest.raises(ValueError):
        read_png(path)
    (tmp_path / "not.png").write_bytes(b"hello")
    with pytest.raises(ValueError):
        read_png(str(tmp_path / "not.png"))


def test_contact_sheet():
    from hyperpocket_amd.utils.render import contact_sheet
    images = torch.arange(5 * 2 * 3 * 3, dtype=torch.int64).reshape(5, 2, 3, 3).to(torch.uint8)
    sheet = contact_sheet(images, 3, background=(9, 8, 7))
    assert sheet.shape == (4, 9, 3) and sheet.dtype == torch.uint8
    for i in range(5):
        r, c = divmod(i, 3)
        assert torch.equal(sheet[r * 2:(r + 1) * 2, c * 3:(c + 1) * 3], images[i])
    assert torch.equal(sheet[2:, 6:], torch.tensor([9, 8, 7], dtype=torch.uint8).expand(2, 3, 3))
    assert torch.equal(contact_sheet(images[:4], 2)[2:, 3:], images[3])                   # no padding needed


def test_package_imports_neither_pillow_nor_matplotlib():
    import glob
    import re
    for path in glob.glob(os.path.join(PKG_DIR, "hyperpocket_amd", "**", "*.py"), recursive=True):
        assert not re.search(r"^\s*(from|import)\s+(PIL|matplotlib)\b", open(path).read(), flags=re.M), path


def test_render_has_no_cpu_path():
    from hyperpocket_amd import HipExtensionError, ops
    with pytest.raises(HipExtensionError):
        ops.render_points(torch.zeros(1, 4, 3), [4], [(1, 2, 3)], [1], torch.zeros(1, 3, 4), (8, 8))


# ------------------------------------------------------------------------------------------------
# C ABI without a GPU
# ------------------------------------------------------------------------------------------------
class Plan(ctypes.Structure):  # HpRenderPlan
    _fields_ = [("tile_w", ctypes.c_int), ("tile_h", ctypes.c_int), ("tiles_x", ctypes.c_int), ("tiles_y", ctypes.c_int),
                ("tiles", ctypes.c_int), ("threads", ctypes.c_int), ("lds_bytes", ctypes.c_int),
                ("workgroups", ctypes.c_longlong)]


def _render(lib, B=1, n=4, V=1, L=2, ends=(2, 4), radius2=(1, 2), fog=96, W=8, H=8, null=()):
    """hp_render_points with fake non-null pointers: every case here must be turned away before anything is read."""
    fake = ctypes.c_void_p(4096)
    arg = lambda name, value: None if name in null else value
    return lib.hp_render_points(B, n, arg("points", fake), V, arg("views", fake), L,
                                arg("layer_ends", (ctypes.c_int * len(ends))(*ends)),
                                arg("palette", (ctypes.c_ubyte * (3 * max(len(ends), 1)))()),
                                arg("radius2", (ctypes.c_int * len(radius2))(*radius2)), fog,
                                arg("background", (ctypes.c_ubyte * 3)()), W, H, arg("image", fake), None, None)


BAD = [dict(B=0), dict(B=-1), dict(n=0, ends=(0, 0)), dict(V=0), dict(W=0), dict(H=0), dict(W=4097), dict(H=4097),
       dict(L=0), dict(L=9, ends=(0,) * 8 + (4,), radius2=(0,) * 9), dict(ends=(3, 2)), dict(ends=(2, 3)), dict(ends=(2, 5)),
       dict(ends=(-1, 4)), dict(radius2=(1, 65)), dict(radius2=(-1, 2)), dict(fog=-1), dict(fog=256),
       dict(null=("points",)), dict(null=("views",)), dict(null=("layer_ends",)), dict(null=("palette",)),
       dict(null=("radius2",)), dict(null=("background",)), dict(null=("image",))]


@pytest.mark.parametrize("case", BAD, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c in BAD])
def test_invalid_arguments_return_minus_one_before_any_hip_call(lib, case):
    assert _render(lib, **case) == -1


def test_too_many_workgroups_for_one_grid_dimension_is_refused(lib):
    assert _render(lib, B=1 << 20, V=1 << 8, W=4096, H=4096) == -1


@pytest.mark.parametrize("W,H", [(1, 1), (128, 128), (129, 130), (4096, 4096), (500, 500), (37, 53)])
def test_plan_answers_on_the_host_and_its_tiles_cover_the_image(lib, W, H):
    try:
        for side in (0, 8, 16, 32, 64, 128):
            before = lib.hp_render_points_set_tile(side)
            plan = Plan()
            assert lib.hp_render_points_plan(3, 2, W, H, ctypes.byref(plan)) == 0
            assert before in (0, 8, 16, 32, 64, 128)
            assert 1 <= plan.tile_w <= min(W, 128) and 1 <= plan.tile_h <= min(H, 128)
            if side:
                assert (plan.tile_w, plan.tile_h) == (min(side, W), min(side, H))
            assert plan.tiles == plan.tiles_x * plan.tiles_y and plan.workgroups == 6 * plan.tiles
            assert plan.tiles_x * plan.tile_w >= W > (plan.tiles_x - 1) * plan.tile_w      # covered, no tile wholly outside
            assert plan.tiles_y * plan.tile_h >= H > (plan.tiles_y - 1) * plan.tile_h
            assert plan.lds_bytes == 8 * plan.tile_w * plan.tile_h <= 160 * 1024           # one 64-bit key per pixel
            assert plan.threads % 64 == 0 and 64 <= plan.threads <= 1024
    finally:
        lib.hp_render_points_set_tile(0)
    assert lib.hp_render_points_set_tile(48) == -1 and lib.hp_render_points_set_tile(-1) == -1
    assert lib.hp_render_points_set_tile(0) == 0                   # the refused values changed nothing
    plan = Plan()
    for bad in ((0, 1, W, H), (1, 0, W, H), (1, 1, 0, H), (1, 1, W, 4097)):
        assert lib.hp_render_points_plan(*bad, ctypes.byref(plan)) == -1
    assert lib.hp_render_points_plan(1, 1, W, H, None) == -1
