"""The law of the point-cloud renderer (csrc/render.hip is bit-equal to it), in numpy and Python integers only.

One image is made from points (n,3) float32, a view M (3,4) float32, L layers given by cumulative ends (point i belongs to the
first layer whose end exceeds i; empty layers allowed; the last end is n), per layer a colour (3 x uint8) and an integer
radius2 in [0, 64], fog in [0, 255], a background colour and the size (W, H).

  projection  per row k of M, in float32, one rounding per operation:  t_k = ((M[k,0]*x + M[k,1]*y) + M[k,2]*z) + M[k,3]
              -> u, v, w
  cull        dropped if any of u, v, w is not finite, or unless -9 <= u < W+9 and -9 <= v < H+9 (float comparisons)
  raster      px = floor(u), py = floor(v), zq = int(min(max(floor(w * 2^24), 0), 2^24 - 1)) with the clamps in float
  key         (zq << 32) | i
  splat       every integer (dx,dy) with dx^2 + dy^2 <= radius2[layer(i)]: pixel (px+dx, py+dy), if inside the image, takes
              min(old, key) — the nearest depth wins, at equal quantised depth the lower index
  resolve     untouched: background, ids -1.  Otherwise shade = 255 - (((zq >> 16) * fog) >> 8), each channel
              (palette[layer][c] * shade + 127) // 255, ids = i.

Returns image (H,W,3) uint8 and ids (H,W) int32."""
import numpy as np

DEPTH_ONE = 1 << 24
MARGIN = np.float32(9.0)
EMPTY = (1 << 64) - 1


def project(points, M):
    """u, v, w (n,) float32 of points (n,3) under M (3,4): products and sums rounded one by one, left to right."""
    p, M = np.asarray(points, np.float32).reshape(-1, 3), np.asarray(M, np.float32)
    with np.errstate(all="ignore"):
        return tuple(((M[k, 0] * p[:, 0] + M[k, 1] * p[:, 1]) + M[k, 2] * p[:, 2]) + M[k, 3] for k in range(3))


def layer_of(i, layer_ends):
    for l, end in enumerate(layer_ends):
        if end > i:
            return l
    raise ValueError(f"point {i} lies past the last layer end")


def shade(zq, fog):
    return 255 - (((zq >> 16) * fog) >> 8)


def colour(rgb, zq, fog):
    s = shade(zq, fog)
    return [(int(c) * s + 127) // 255 for c in rgb]


def disc(radius2):
    r = int(np.sqrt(radius2))
    return [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= radius2]


def keys(points, M, size):
    """Per point (px, py, zq) as Python ints, or None where the point is culled."""
    W, H = size
    u, v, w = project(points, M)
    out = []
    with np.errstate(all="ignore"):
        keep = np.isfinite(u) & np.isfinite(v) & np.isfinite(w) & (u >= -MARGIN) & (u < np.float32(W) + MARGIN) \
            & (v >= -MARGIN) & (v < np.float32(H) + MARGIN)
        zf = np.minimum(np.maximum(np.floor(w * np.float32(DEPTH_ONE)), np.float32(0)), np.float32(DEPTH_ONE - 1))
    for i in range(len(u)):
        out.append((int(np.floor(u[i])), int(np.floor(v[i])), int(zf[i])) if keep[i] else None)
    return out


def render(points, M, layer_ends, palette, radius2, size, fog, background):
    W, H = size
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(points)
    layer_ends = [int(e) for e in layer_ends]
    assert layer_ends and layer_ends[-1] == n and all(a <= b for a, b in zip([0] + layer_ends, layer_ends))
    assert all(0 <= int(r) <= 64 for r in radius2) and 0 <= fog <= 255
    discs = [disc(int(r)) for r in radius2]
    zbuf = [[EMPTY] * W for _ in range(H)]
    for i, hit in enumerate(keys(points, M, size)):
        if hit is None:
            continue
        px, py, zq = hit
        key = (zq << 32) | i
        for dx, dy in discs[layer_of(i, layer_ends)]:
            x, y = px + dx, py + dy
            if 0 <= x < W and 0 <= y < H and key < zbuf[y][x]:
                zbuf[y][x] = key
    return resolve(zbuf, layer_ends, palette, fog, background)


def resolve(zbuf, layer_ends, palette, fog, background):
    """image and ids of a buffer of keys (H rows of W Python ints): the resolve step over whole arrays, in int64."""
    z = np.array(zbuf, dtype=np.uint64)
    hit = z != np.uint64(EMPTY)
    i = (z & np.uint64(0xFFFFFFFF)).astype(np.int64)
    zq = (z >> np.uint64(32)).astype(np.int64)
    layer = np.minimum(np.searchsorted(np.asarray(layer_ends, np.int64), i, side="right"), len(layer_ends) - 1)
    lit = (np.asarray(palette, np.int64)[layer] * shade(zq, fog)[..., None] + 127) // 255
    image = np.where(hit[..., None], lit, np.asarray(background, np.int64)).astype(np.uint8)
    ids = np.where(hit, i, -1).astype(np.int32)
    return image, ids


def render_batch(points, views, layer_ends, palette, radius2, size, fog, background):
    """points (B,n,3), views (V,3,4) -> image (B,V,H,W,3) uint8, ids (B,V,H,W) int32."""
    points, views = np.asarray(points, np.float32), np.asarray(views, np.float32)
    out = [[render(p, M, layer_ends, palette, radius2, size, fog, background) for M in views] for p in points]
    return (np.stack([np.stack([o[0] for o in row]) for row in out]), np.stack([np.stack([o[1] for o in row]) for row in out]))
