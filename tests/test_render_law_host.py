"""CPU suite for tests/render_law.py, the law csrc/render.hip is held to: a 5 x 5 image worked out by hand, the shade
formula at its ends, and the cull and depth clamps — so that the checker itself is checked against something that is not code."""
import numpy as np

import render_law

IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)     # u = x, v = y, w = z


def test_hand_computed_image():
    """Three points on a 5 x 5 image, layer 0 = points 0 and 1 (radius2 1: a plus of 5 pixels), layer 1 = point 2 (radius2 0).
    Point 0 sits in pixel (0,1) at w = 1/8 + 2^-26, so its plus loses its left arm to the image edge; point 1 sits in pixel
    (1,1) at w = 1/8, truly nearer but with the same zq = 2^21, so the two pixels both cover go to the lower index; point 2
    sits in pixel (1,1) at w = 1/16 and takes that one pixel from both."""
    points = np.array([[0.5, 1.5, 0.125 + 2.0 ** -26], [1.25, 1.75, 0.125], [1.9, 1.0, 0.0625]], np.float32)
    assert points[0, 2] != points[1, 2]
    image, ids = render_law.render(points, IDENTITY, [2, 3], [(200, 100, 50), (10, 250, 30)], [1, 0], (5, 5), 255, (1, 2, 3))
    want_ids = np.array([[0, 1, -1, -1, -1],
                         [0, 2, 1, -1, -1],
                         [0, 1, -1, -1, -1],
                         [-1, -1, -1, -1, -1],
                         [-1, -1, -1, -1, -1]], np.int32)
    assert ids.dtype == np.int32 and image.dtype == np.uint8 and image.shape == (5, 5, 3)
    assert np.array_equal(ids, want_ids)
    # zq = 2^21: (2^21 >> 16) = 32, (32 * 255) >> 8 = 31, shade 224; zq = 2^20: 16, (16 * 255) >> 8 = 15, shade 240
    near, far, back = (9, 235, 28), (176, 88, 44), (1, 2, 3)       # (c * shade + 127) // 255, by hand
    for y in range(5):
        for x in range(5):
            want = back if want_ids[y, x] < 0 else near if want_ids[y, x] == 2 else far
            assert tuple(image[y, x]) == want, (x, y)


def test_shade_formula():
    top = (1 << 24) - 1
    for fog in (0, 96, 255):
        assert render_law.shade(0, fog) == 255
    assert [render_law.shade(top, fog) for fog in (0, 96, 255)] == [255, 160, 1]           # 255 - ((255 * fog) >> 8)
    assert [render_law.shade(1 << 23, fog) for fog in (0, 96, 255)] == [255, 207, 128]     # 255 - ((128 * fog) >> 8)
    assert render_law.colour((255, 128, 0), top, 96) == [160, 80, 0]                       # (128 * 160 + 127) // 255 = 80
    assert render_law.colour((255, 128, 1), top, 255) == [1, 1, 0]                         # (128 + 127) // 255 = 1


def test_cull_and_depth_clamps():
    """The 9-pixel margin is a float comparison on u and v before any conversion; w only has to be finite and is clamped."""
    W, H = 20, 10
    rows = [(-9.0, 0.0, 0.5, True), (np.nextafter(np.float32(-9.0), np.float32(-10.0)), 0.0, 0.5, False),
            (np.nextafter(np.float32(29.0), np.float32(0.0)), 0.0, 0.5, True), (29.0, 0.0, 0.5, False),
            (0.0, -9.0, 0.5, True), (0.0, 19.0, 0.5, False), (0.0, np.nextafter(np.float32(19.0), np.float32(0.0)), 0.5, True),
            (np.nan, 0.0, 0.5, False), (0.0, np.inf, 0.5, False), (0.0, 0.0, -np.inf, False), (0.0, 0.0, np.nan, False),
            (3e9, 0.0, 0.5, False), (0.0, 1e30, 0.5, False), (0.0, 0.0, 1e30, True), (0.0, 0.0, -3e9, True)]
    got = render_law.keys(np.array([r[:3] for r in rows], np.float32), IDENTITY, (W, H))
    for r, g in zip(rows, got):
        assert (g is not None) == r[3], r
    assert got[0][:2] == (-9, 0) and got[2][:2] == (28, 0) and got[6][:2] == (0, 18)
    assert got[13][2] == (1 << 24) - 1 and got[14][2] == 0                                 # clamped, not wrapped
    # w = 1 - 2^-24 is the largest depth below 1: the last quantum
    assert render_law.keys(np.array([[0, 0, 1 - 2.0 ** -24]], np.float32), IDENTITY, (W, H))[0][2] == (1 << 24) - 1


def test_a_point_outside_by_less_than_its_radius_still_reaches_the_image():
    image, ids = render_law.render(np.array([[-2.5, 1.5, 0.5]], np.float32), IDENTITY, [1], [(9, 9, 9)], [9], (4, 4), 0, (0, 0, 0))
    assert ids[1, 0] == 0 and ids[1, 1] == -1 and (ids[:, 0] >= 0).sum() == 1             # px = -3, r = 3: column 0 at dy = 0 only
    _, ids = render_law.render(np.array([[-2.5, 1.5, 0.5]], np.float32), IDENTITY, [1], [(9, 9, 9)], [8], (4, 4), 0, (0, 0, 0))
    assert (ids == -1).all()


def test_empty_layers_and_layer_lookup():
    assert [render_law.layer_of(i, [0, 2, 2, 5]) for i in range(5)] == [1, 1, 3, 3, 3]
    assert len(render_law.disc(0)) == 1 and len(render_law.disc(1)) == 5 and len(render_law.disc(2)) == 9
    assert len(render_law.disc(4)) == 13 and len(render_law.disc(9)) == 29 and len(render_law.disc(64)) == 197
