"""Pictures of point clouds, drawn on the device: where the reference's utils/pcutil.py plot_3d_point_cloud makes a
matplotlib 3-D scatter per cloud, ops.render_points draws B clouds as depth-buffered, depth-shaded splats in one launch and
write_png stores the result with the standard library alone.  What is drawn is the points and, optionally, a second layer of
highlighted points; titles, axes, ticks and colour bars are not drawn — there is no font here.  Pillow and matplotlib are
never imported."""
import math
import os
import struct
import zlib

import numpy as np

import torch

from .. import ops

DEFAULT_ELEV, DEFAULT_AZIM = 10.0, 240.0       # the reference's camera (utils/pcutil.py:110-111)
DEFAULT_SIZE = (500, 500)                      # (W, H): its figsize (5, 5) at 100 dpi
DEFAULT_PALETTE = ((31, 119, 180), (214, 39, 40))      # the points, the overlay (red, as the reference's x1, y1, z1)
DEFAULT_RADIUS2 = 2                            # a 3 x 3 disc: 9 pixels
DEFAULT_OVERLAY_RADIUS2 = 9                    # 29 pixels, about three times the marker area, as the reference draws it
DEFAULT_FOG = 96                               # the farthest points keep 5/8 of their colour
DEFAULT_BACKGROUND = (255, 255, 255)
PNG_LEVEL = 1                                  # zlib level of write_png: DESIGN.md 3j has the timings behind it


def view_matrix(elev=DEFAULT_ELEV, azim=DEFAULT_AZIM, size=DEFAULT_SIZE, lo=-0.5, hi=0.5, extent=None):
    """The (3,4) float32 matrix that takes a point to (u, v, w): pixel column, pixel row and depth in [0, 1), nearest 0 — an
    orthographic camera at elevation `elev` and azimuth `azim` (degrees, matplotlib's view_init) looking at the centre of the
    cube [lo, hi]^3.  Computed in fp64 and rounded once.  With e = (cos el cos az, cos el sin az, sin el) the direction of the
    eye, r = (-sin az, cos az, 0) the screen's right and up = e x r, c the cube's centre and s = min(W, H) / 2 / extent:
    u = W/2 + s r.(p - c), v = H/2 - s up.(p - c), w = 0.5 - e.(p - c) / (2 extent).  `extent`, the distance from the centre
    that reaches the edge of the shorter side, defaults to half the cube's diagonal: the whole cube is on screen under every
    angle.  The three world axes point the same way on screen as under matplotlib's orthographic view."""
    W, H = size
    el, az = math.radians(elev), math.radians(azim)
    e = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    r = np.array([-math.sin(az), math.cos(az), 0.0])
    up = np.cross(e, r)
    c = np.full(3, (lo + hi) / 2.0)
    if extent is None:
        extent = (hi - lo) / 2.0 * math.sqrt(3.0)
    s = min(W, H) / 2.0 / extent
    M = np.empty((3, 4), np.float64)
    M[0, :3], M[0, 3] = s * r, W / 2.0 - s * c.dot(r)
    M[1, :3], M[1, 3] = -s * up, H / 2.0 + s * c.dot(up)
    M[2, :3], M[2, 3] = -e / (2.0 * extent), 0.5 + c.dot(e) / (2.0 * extent)
    return M.astype(np.float32)


DEFAULT_VIEW = view_matrix()


def _device_clouds(clouds, device=None):
    """(B,n,3) float32 contiguous on the device, from a tensor on any device or an array; (n,3) counts as one cloud."""
    t = clouds if isinstance(clouds, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(clouds, np.float32))
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if not t.is_cuda:
        t = t.to(device if device is not None else "cuda")
    return t.detach().to(torch.float32).contiguous()


def render_clouds(clouds, overlay=None, views=None, size=DEFAULT_SIZE, palette=DEFAULT_PALETTE, radius2=DEFAULT_RADIUS2,
                  overlay_radius2=DEFAULT_OVERLAY_RADIUS2, fog=DEFAULT_FOG, background=DEFAULT_BACKGROUND):
    """clouds (B,n,3) and, optionally, overlay (B,m,3) — highlighted points, a second layer of its own colour and radius
    that takes part in the depth test like any other point — under `views` ((V,3,4) or (3,4), array or tensor; default: the
    reference's camera at `size`) -> images (B,V,H,W,3) uint8 on the device, in one launch.  Nothing is synchronised."""
    pts = _device_clouds(clouds)
    ends, radii, colours = [pts.size(1)], [radius2], [palette[0]]
    if overlay is not None:
        over = _device_clouds(overlay, pts.device)
        if over.size(0) != pts.size(0):
            raise ValueError(f"overlay must have one row of points per cloud, got {over.size(0)} for {pts.size(0)}")
        pts = torch.cat([pts, over], 1)
        ends, radii, colours = ends + [pts.size(1)], radii + [overlay_radius2], colours + [palette[1]]
    if views is None:
        views = DEFAULT_VIEW if tuple(size) == DEFAULT_SIZE else view_matrix(size=size)
    if not isinstance(views, torch.Tensor):
        views = torch.from_numpy(np.ascontiguousarray(views, np.float32))
    views = views.to(pts.device, torch.float32).reshape(-1, 3, 4).contiguous()
    return ops.render_points(pts, ends, colours, radii, views, size, fog=fog, background=background)


def contact_sheet(images, columns, background=DEFAULT_BACKGROUND):
    """images (N,H,W,3) -> one (rows*H, columns*W, 3) image, row-major, the last row filled up with `background`: reshapes
    only, on whichever device the images are."""
    N, H, W, C = images.shape
    rows = -(-N // columns)
    if rows * columns > N:
        pad = torch.tensor(background, dtype=images.dtype, device=images.device).expand(rows * columns - N, H, W, C)
        images = torch.cat([images, pad])
    return images.reshape(rows, columns, H, W, C).permute(0, 2, 1, 3, 4).reshape(rows * H, columns * W, C)


_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, array, level=PNG_LEVEL):
    """An (H,W,3) uint8 array (or CPU tensor) as an 8-bit RGB PNG: one IDAT chunk, every row filter type 0.  Returns path."""
    a = np.ascontiguousarray(array.numpy() if isinstance(array, torch.Tensor) else array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"an (H,W,3) uint8 image is required, got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), np.uint8)              # a filter byte (0) in front of every row
    rows[:, 1:] = a.reshape(H, 3 * W)
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b""))
    return path


def read_png(path):
    """The (H,W,3) uint8 array of an 8-bit RGB, non-interlaced PNG whose rows all have filter type 0 — what write_png
    writes; anything else, a bad signature or a bad CRC is a ValueError."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f"{path}: not a PNG file")
    pos, header, idat = 8, None, []
    while pos < len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + length]
        if struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])[0] != zlib.crc32(kind + body) & 0xFFFFFFFF:
            raise ValueError(f"{path}: bad CRC in chunk {kind!r}")
        pos += 12 + length
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if header is None or header[2:] != (8, 2, 0, 0, 0):
        raise ValueError(f"{path}: only 8-bit RGB, non-interlaced PNGs are read")
    W, H = header[:2]
    rows = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    if rows.size != H * (1 + 3 * W):
        raise ValueError(f"{path}: {rows.size} bytes of image data for {W} x {H}")
    rows = rows.reshape(H, 1 + 3 * W)
    if rows[:, 0].any():
        raise ValueError(f"{path}: only rows of filter type 0 are read")
    return rows[:, 1:].reshape(H, W, 3).copy()


def save_plot(X, epoch, k, results_dir, t):
    """The reference's utils/util.py save_plot by name and path: the cloud X (3,n) — a tensor on any device or an array —
    drawn under the default view into results_dir/f'{epoch}_{k}_{t}.png'.  Its title is not drawn.  Returns the path."""
    X = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X, np.float32))
    image = render_clouds(X.detach().t().unsqueeze(0))
    return write_png(os.path.join(results_dir, f'{epoch}_{k}_{t}.png'), image[0, 0].cpu())
