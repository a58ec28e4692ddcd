"""Test-time inputs that live on the GPU: partial scans of different sizes, packed once as a ragged set (points (T,3) +
offsets (S+1)) and turned into fixed-size encoder inputs there by ops.prepare_scans (csrc/scan_prep.hip) — the resampling
of the reference's 3D-EPN test split (datasets/shapenet_3depn.py:18-49,107-123) and of its real-scan dataset
(datasets/real_data.py, utils/util.py:95-100) without a per-item numpy step.

    data = DeviceScanDataset.from_npy_dir("scans/")                  # object*.npy [+ scen*.npy, object_box*.npy]
    for existing, ids, _ in ScanBatcher(data, 8, target=1024, normalize=True):
        code = model.encode_existing(existing)
        ...
    in_scene = data.inverse_scale_to_scene(0, completion)            # back in the scan's own coordinates

    data = DeviceScanDataset.from_npy_dir("scans/", outliers=(16, 2.0))   # flying pixels dropped before boxes and batches
    clean = data.without_outliers(k=16, ratio=2.0)                   # the same, from a dataset that exists
    clean = clean.without_plane(threshold=0.01)                      # the floor or table top goes (csrc/plane.hip); .planes has it
    clean = clean.without_edges(k=16, max_curvature=0.05)            # the mixed pixels of depth edges go (csrc/normals.hip)
    main = clean.keep_clusters(radius=0.05)                          # each scan's largest connected piece (csrc/clusters.hip)
    normal, curvature = main.normals(k=16, viewpoint=(0, 0, 0))      # which way the surface faces, seen from the sensor

    big = DeviceScanDataset.from_npy_dir("sensor/")                  # hundreds of thousands of rows per scan
    thin = big.thinned(voxel=0.01)                                   # first: one row per 1 cm cell (csrc/voxels.hip), even density
    thin = big.thinned(max_points=32768)                             # ... or the finest grid that leaves at most 32768 rows a scan
    main = thin.without_plane(0.01).without_outliers().keep_clusters(radius=0.05)      # now within the filters' caps
    objects = scene_data.split_clusters(radius=0.05, min_points=200) # scene in, objects out: every piece a scan of its own
    whole = big.with_search("grid")                                  # ... or the whole sensor scan on its own rows: the same
    clean = whole.without_outliers().without_edges(max_curvature=0.05)     # neighbours behind a grid (csrc/knn_grid.hip), scans of
    normal, curvature = clean.normals(k=16, viewpoint=(0, 0, 0))     # up to 2^22 rows; the setting travels with the filtered sets
    whole = main.merged_views([[0, 1, 2]], max_dist=0.05)            # last: captures of one object in one frame (csrc/align.hip)
    posed = main.aligned_to(template, max_dist=0.1, yaw=24)          # ... or every scan onto a template; .poses has the motions
    posed = main.aligned_to_surface(template, max_dist=0.1)          # ... refined along the template's normals (csrc/align_plane.hip)

    views = viewpoints_on_sphere(len(clouds) * 4, 2.5, seed=0).reshape(-1, 4, 3)
    partial = DeviceScanDataset.virtual_scans(clouds, views)         # complete clouds as four sensors each would see them
    near = main.seen_from((0, 0, 0), keep="nearest")                 # (csrc/visibility.hip); .gt / .viewpoints travel along

    frames = DeviceScanDataset.from_depth_images(depth, (fx, fy, cx, cy), poses=cam_to_world, masks=instance)   # (B,H,W) uint16
    objects = frames.without_plane(0.01).keep_clusters(0.05)         # (csrc/depth.hip) holes, range, mask and depth edges are
    normal, pixel = objects.row_normals(), objects.row_pixels()      # gone already; .viewpoints and pixel-grid normals come along

ScanBatcher(..., resample="farthest") keeps farthest-point picks (ops.farthest_points, csrc/fps.hip) instead of a uniform
subset: the choice for scans whose density varies over the surface.

Depth images need no conversion: from_depth_images takes what the sensor delivers.  Reading `.ply` / `.h5` files is a one-time
conversion of the user's and not done here.  A ragged `gt` is not kept: bring it to one size up front with
ops.prepare_scans(target=2048).
"""
import os

import numpy as np
import torch

from .. import ops
from .._lib import HipExtensionError


def _pack(scans):
    """A list of (n_i,3) arrays or a (points, offsets) pair -> (points (T,3) float32, offsets (S+1) int64) CPU or GPU tensors."""
    if isinstance(scans, tuple) and len(scans) == 2 and torch.as_tensor(scans[1]).dim() == 1:
        points, offsets = torch.as_tensor(scans[0]), torch.as_tensor(scans[1])
        if offsets.is_floating_point() or offsets.numel() < 2:
            raise ValueError("offsets must be (S+1) integers with S >= 1")
        offsets = offsets.to(torch.int64)
    else:
        scans = [torch.as_tensor(s) for s in scans]
        if not scans:
            raise ValueError("a scan dataset needs at least one scan")
        for i, s in enumerate(scans):
            if s.dim() != 2 or s.size(1) != 3:
                raise ValueError(f"scan {i} must be (n,3), got {tuple(s.shape)}")
        points = torch.cat([s.to(torch.float32) for s in scans])
        offsets = torch.tensor([0] + [s.size(0) for s in scans], dtype=torch.int64).cumsum(0)
    if points.dim() != 2 or points.size(1) != 3:
        raise ValueError(f"points must be (T,3), got {tuple(points.shape)}")
    lengths = (offsets[1:] - offsets[:-1]).cpu()
    if int(offsets[0]) != 0 or int(offsets[-1]) != points.size(0):
        raise ValueError("offsets must run from 0 to the number of points")
    if int(lengths.min()) < 1:
        raise ValueError("every scan needs at least one point")
    if int(lengths.max()) > ops.SCAN_MAX_POINTS:
        raise ValueError(f"a scan holds at most {ops.SCAN_MAX_POINTS} points")
    return points.to(torch.float32), offsets


def viewpoints_on_sphere(count, radius, seed, center=(0, 0, 0)):
    """`count` sensor positions on the sphere of `radius` about `center`, (count,3) float32 on the host: numpy's
    default_rng(seed).standard_normal((count, 3)) in float64, each row divided by its norm, times radius, plus center.
    Host-side and reproducible: a function of its arguments (and of numpy's generator) alone."""
    if int(count) < 1 or not float(radius) > 0.0:
        raise ValueError(f"count >= 1 and radius > 0 are required, got count = {count}, radius = {radius}")
    n = np.random.default_rng(seed).standard_normal((int(count), 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return (n * float(radius) + np.asarray(center, dtype=np.float64).reshape(1, 3)).astype(np.float32)


class DeviceScanDataset:
    """S partial scans of n_s points each, resident on the device as one ragged set.
    scans: a list of (n_i,3) arrays / tensors, or a (points (T,3), offsets (S+1)) pair; packed and uploaded once.
    gt: optional (S,N,3) complete clouds; names: optional S names; transform: optional (3,3) matrix M, every point p becomes
    M @ p once, here (an axis swap such as 3D-EPN's belongs here, not in the kernel).  scenes / boxes: optional per-scan
    arrays of the real-scan layout, kept on the host until asked for.
    outliers: optional (k, ratio): statistical outlier removal (without_outliers) applied here, before boxes and
    normalisation ever see the points; rows with non-finite values, an error without it, are then dropped with the outliers.
    clusters: optional (radius, min_points): keep_clusters applied after `outliers` and before boxes.
    plane: optional (threshold, trials): without_plane applied before `outliers` and `clusters` — it takes whole scenes.
    A filtered dataset has source_rows (its rows as rows of the set it came from, int64) and kept (rows per scan); both are
    None otherwise.  A dataset made by split_clusters has source_scan (the scan each piece came from, int64), None otherwise.
    A dataset made by without_plane has planes (S,4) float32 and plane_found (S) bool on the device, None otherwise.
    A dataset made by thinned has voxels (S) float32 on the device, the cell edge used per scan, None otherwise.
    A dataset made by seen_from, virtual_scans or from_depth_images has viewpoints (S,3) float32 on the device, the sensor
    positions, None otherwise.  A dataset made by from_depth_images has pixels (T) int64 and pixel_normals (T,3) float32, aligned
    with its rows as built (row_pixels / row_normals follow them through the filters), None otherwise.
    A dataset made by aligned_to, merged_views or their _surface variants has poses, pose_ok and pose_rms on the host (merged_views: view_rows too),
    None otherwise.  search is "brute" or, on a dataset made by with_search("grid"), "grid": how the neighbour searches run."""

    def __init__(self, scans, gt=None, names=None, transform=None, device=None, scenes=None, obj_boxes=None, outliers=None,
                 clusters=None, plane=None):
        points, offsets = _pack(scans)
        if device is None:
            device = points.device if points.is_cuda else torch.device("cuda", torch.cuda.current_device())
        points = points.to(device)
        if outliers is None and not bool(torch.isfinite(points).all()):    # once, at construction: the only check that reads the data
            raise ValueError("scans contain non-finite values")
        if transform is not None:
            m = torch.as_tensor(transform, dtype=torch.float32).to(device)
            if tuple(m.shape) != (3, 3):
                raise ValueError("transform must be a (3,3) matrix")
            points = points @ m.t()
        self.points = points.contiguous()
        self.offsets = offsets.to(device).contiguous()
        self.offsets_host = offsets.cpu()                          # host copies: shapes are known without a synchronisation
        self.lengths = self.offsets_host[1:] - self.offsets_host[:-1]
        S = self.lengths.numel()
        self.gt = None
        if gt is not None:
            g = torch.as_tensor(gt)
            if g.dim() != 3 or g.size(0) != S or g.size(2) != 3:
                raise ValueError(f"gt must be (S,N,3) with S = {S}, got {tuple(g.shape)}")
            self.gt = g.to(device=device, dtype=torch.float32).contiguous()
        self.names = None if names is None else [str(n) for n in names]
        if self.names is not None and len(self.names) != S:
            raise ValueError("names must have one entry per scan")
        for what, seq in (("scenes", scenes), ("obj_boxes", obj_boxes)):
            if seq is not None and len(seq) != S:
                raise ValueError(f"{what} must have one entry per scan")
        self.scenes, self.obj_boxes = scenes, obj_boxes
        self._boxes = None
        self.source_rows = self.kept = self.source_scan = None
        self.planes = self.plane_found = self.voxels = self.viewpoints = None
        self.poses = self.pose_ok = self.pose_rms = self.view_rows = None
        self.search = "brute"                                      # with_search("grid") changes it
        self.pixels = self.pixel_normals = None                    # from_depth_images sets them
        self.volume = None                                         # fused_depth_images sets it
        if plane is not None:
            threshold, trials = plane
            self._drop_plane(threshold, trials=trials)
        if outliers is not None:
            k, ratio = outliers
            self._drop_outliers(k, ratio)
        if clusters is not None:
            radius, min_points = clusters
            self._drop_clusters(radius, min_points)

    def _search_cap(self, search, what):
        """Checks `search` (None: the dataset's setting) and, for "grid", the cap of the grid-backed search
        (ops.knn_points_grid); True for "grid"."""
        if search is None:
            search = self.search
        if search not in ("brute", "grid"):
            raise ValueError(f'search must be "brute" or "grid", got {search!r}')
        if search == "brute":
            return False
        longest = int(self.lengths.argmax())
        if int(self.lengths[longest]) > ops.KNN_GRID_MAX_POINTS:
            raise ValueError(f"scan {self._label(longest)} holds {int(self.lengths[longest])} points: {what} by the grid-backed search "
                             f"takes scans of at most {ops.KNN_GRID_MAX_POINTS} points and does not subsample; thin it first")
        return True

    def _drop_outliers(self, k, ratio, search=None):
        """Replaces the ragged set by its kept rows (ops.scan_outliers, or ops.scan_outliers_grid under search="grid"), in
        scan order.  One host synchronisation."""
        if not self.points.is_cuda:
            raise HipExtensionError("outlier removal needs a dataset on the GPU — it has no CPU path")
        if self._search_cap(search, "outlier removal"):
            keep, _, kept = ops.scan_outliers_grid(self.points, self.offsets, k, ratio)
            self._keep_rows(keep, kept, f"outlier removal (k = {k}, ratio = {ratio})")
            return
        longest = int(self.lengths.argmax())
        if int(self.lengths[longest]) > ops.KNN_MAX_POINTS:
            raise ValueError(f"scan {self._label(longest)} holds {int(self.lengths[longest])} points: outlier removal takes scans of at "
                             f"most {ops.KNN_MAX_POINTS} points (brute-force neighbours) and does not subsample; thin it first")
        keep, _, kept = ops.scan_outliers(self.points, self.offsets, k, ratio)
        self._keep_rows(keep, kept, f"outlier removal (k = {k}, ratio = {ratio})")

    def _normals(self, k, viewpoint, what):
        """(normal, curvature, count) of ops.scan_normals over the resident set, after the checks the host can make; with
        the dataset's search "grid" (with_search) the lists come from ops.knn_points_grid."""
        if not self.points.is_cuda:
            raise HipExtensionError(f"{what} needs a dataset on the GPU — it has no CPU path")
        if self._search_cap(None, what):
            if viewpoint is not None:
                viewpoint = torch.as_tensor(viewpoint, dtype=torch.float32).to(self.device).contiguous()
            index, _ = ops.knn_points_grid(self.points, self.offsets, k)
            return ops.scan_normals(self.points, self.offsets, k, viewpoints=viewpoint, index=index)
        longest = int(self.lengths.argmax())
        if int(self.lengths[longest]) > ops.KNN_MAX_POINTS:
            raise ValueError(f"scan {self._label(longest)} holds {int(self.lengths[longest])} points: {what} takes scans of at "
                             f"most {ops.KNN_MAX_POINTS} points (brute-force neighbours) and does not subsample; thin it first")
        if viewpoint is not None:
            viewpoint = torch.as_tensor(viewpoint, dtype=torch.float32).to(self.device).contiguous()
        return ops.scan_normals(self.points, self.offsets, k, viewpoints=viewpoint)

    def _drop_edges(self, k, max_curvature):
        """Replaces the ragged set by the rows with curvature <= max_curvature (ops.scan_normals), in scan order.  One host
        synchronisation."""
        max_curvature = float(max_curvature)
        if not 0.0 <= max_curvature <= 1.0 / 3.0:
            raise ValueError(f"0 <= max_curvature <= 1/3 is required (the surface variation's range), got {max_curvature}")
        _, curvature, _ = self._normals(k, None, "edge removal")
        keep = curvature <= max_curvature                          # a NaN never passes
        kept = torch.zeros(len(self), dtype=torch.int64, device=self.device).index_add_(0, self._scan_of_rows(), keep.to(torch.int64))
        self._keep_rows(keep, kept, f"edge removal (k = {k}, max_curvature = {max_curvature})")

    def _keep_rows(self, keep, kept, what):
        """Replaces the ragged set by the rows with keep (T) != 0, in scan order; kept (S): their number per scan, on the
        device.  Reading it is the one host synchronisation.  Raises ValueError naming the scan that `what` would empty."""
        rows = torch.nonzero(keep).squeeze(1)                      # ascending: scan order, and the order within a scan
        kept = kept.cpu().to(torch.int64)
        empty = torch.nonzero(kept == 0)
        if empty.numel():
            raise ValueError(f"scan {self._label(int(empty[0]))} would be left without points by {what}")
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64), kept.cumsum(0)])
        self.source_rows = rows if self.source_rows is None else self.source_rows[rows]
        self.points = self.points[rows].contiguous()
        self.offsets, self.offsets_host = offsets.to(self.points.device).contiguous(), offsets
        self.lengths, self.kept = kept, kept
        self._boxes = None

    def _clusters(self, radius, what):
        """(label, size, clusters, largest) of ops.scan_clusters over the resident set, after the checks the host can make."""
        if not self.points.is_cuda:
            raise HipExtensionError(f"{what} needs a dataset on the GPU — it has no CPU path")
        longest = int(self.lengths.argmax())
        if int(self.lengths[longest]) > ops.CLUSTER_MAX_POINTS:
            raise ValueError(f"scan {self._label(longest)} holds {int(self.lengths[longest])} points: {what} takes scans of at most "
                             f"{ops.CLUSTER_MAX_POINTS} points (the forest of a scan lives in one workgroup's LDS) and does not "
                             f"subsample; thin it first")
        return ops.scan_clusters(self.points, self.offsets, radius, max_points=int(self.lengths[longest]))

    def _scan_of_rows(self):
        """(T) int64: the scan of every resident row."""
        return torch.repeat_interleave(torch.arange(len(self), device=self.device), self.lengths.to(self.device),
                                       output_size=self.points.size(0))    # the size is known: no synchronisation

    def _drop_clusters(self, radius, min_points):
        """Replaces the ragged set by the rows of each scan's largest component (min_points None) or of every component of at
        least min_points rows (ops.scan_clusters), in scan order.  One host synchronisation."""
        label, size, _, largest = self._clusters(radius, "cluster extraction")
        if min_points is None:
            keep = (label == largest[self._scan_of_rows()]) & (label >= 0)     # a scan without a present row: -1 == -1
            what = f"cluster extraction (radius = {radius})"
        else:
            if int(min_points) < 1:
                raise ValueError("min_points >= 1 is required")
            keep = size >= int(min_points)
            what = f"cluster extraction (radius = {radius}, min_points = {int(min_points)})"
        kept = torch.zeros(len(self), dtype=torch.int64, device=self.device).index_add_(0, self._scan_of_rows(), keep.to(torch.int64))
        self._keep_rows(keep, kept, what)

    def _drop_plane(self, threshold, trials=512, seed=0, min_inliers=3, min_share=0.2, refine=True):
        """Replaces the ragged set by the rows off each scan's dominant plane (ops.scan_plane) and sets planes and
        plane_found.  One host synchronisation, and with refine a read of the moments before it."""
        if not self.points.is_cuda:
            raise HipExtensionError("plane removal needs a dataset on the GPU — it has no CPU path")
        S, dev = len(self), self.device
        res = ops.scan_plane(self.points, self.offsets, threshold, trials=trials, seed=seed, min_inliers=min_inliers,
                             min_share=min_share)
        found = res["found"] != 0
        scan = self._scan_of_rows()
        if refine:
            anchor = self.points[(self.offsets[:-1] + res["sample"][:, 0].clamp(min=0)).clamp(max=self.points.size(0) - 1)]
            planes = ops.plane_from_moments(res["moments"], res["shift"], res["sample_plane"], anchor)     # reads them: host
            planes = torch.from_numpy(planes).to(torch.float32).to(dev)
            planes = torch.where(found.unsqueeze(1), planes, torch.full_like(planes, float("nan"))).contiguous()
            dist, keep, _ = ops.scan_plane_side(self.points, self.offsets, planes, threshold)
        else:
            sp = res["sample_plane"]
            planes = sp / sp[:, :3].square().sum(1, keepdim=True).sqrt()
            planes = torch.where(found.unsqueeze(1), planes, torch.full_like(planes, float("nan"))).contiguous()
            keep = res["inlier"] == 0
            pl = planes[scan]
            dist = (self.points * pl[:, :3]).sum(1) + pl[:, 3]
        keep = keep.to(torch.bool) | ~found[scan]                  # a scan without a plane is left whole
        kept = torch.zeros(S, dtype=torch.int64, device=dev).index_add_(0, scan, keep.to(torch.int64))
        # most of the kept rows on the positive side: one reduction over the signs of their distances
        side = torch.sign(dist).nan_to_num_(0.0) * keep
        votes = torch.zeros(S, dtype=torch.float32, device=dev).index_add_(0, scan, side)
        self.planes = torch.where((votes < 0).unsqueeze(1), -planes, planes)
        self.plane_found = found
        self._keep_rows(keep, kept, f"plane removal (threshold = {threshold}, trials = {trials})")

    THIN_ROUNDS = 16                                               # bisection steps of thinned(max_points=...)

    def _thin(self, voxel, max_points, keep, origin):
        """Replaces the ragged set by one row per occupied cell (ops.scan_voxels) and sets voxels.  One host synchronisation."""
        if (voxel is None) == (max_points is None):
            raise ValueError("exactly one of voxel and max_points is required")
        if keep not in ("center", "first"):
            raise ValueError(f'keep must be "center" or "first", got {keep!r}')
        if origin is not None and origin != "center":
            raise ValueError(f'origin must be None or "center", got {origin!r}')
        if max_points is not None and int(max_points) < 8:
            raise ValueError(f"max_points >= 8 is required (a grid of two cells per axis), got {max_points}")
        if not self.points.is_cuda:
            raise HipExtensionError("thinning needs a dataset on the GPU — it has no CPU path")
        S, dev = len(self), self.device
        anchor = self.boxes()[0].contiguous() if origin == "center" else None
        advice = 'anchor the grid at the scan with origin="center" or use a larger voxel'
        if voxel is not None:
            res = ops.scan_voxels(self.points, self.offsets, voxel, origin=anchor, keep=keep)
            edge = voxel if isinstance(voxel, torch.Tensor) else torch.full((S,), float(voxel), dtype=torch.float32, device=dev)
            kept, beyond = torch.stack([res["kept"], res["beyond"]]).cpu()         # the host synchronisation
            bad = torch.nonzero(beyond)
            if bad.numel():
                s = int(bad[0])
                raise ValueError(f"scan {self._label(s)} has {int(beyond[s])} rows beyond the grid of {2 * ops.VOXEL_GRID_HALF} "
                                 f"cells per axis: the voxel is too small for the scan's coordinates; {advice}")
            self.voxels = edge.clone()
            self._keep_rows(res["keep"], kept, f"thinning (voxel = {voxel})")
            return
        m = int(max_points)
        scale = self.boxes()[1]
        hi = torch.where(scale == 0, torch.ones_like(scale), scale)
        lo = torch.zeros_like(hi)
        whole = self.lengths <= m                                  # left as they are, bit for bit; known on the host
        if bool(whole.all()):                                      # nothing to thin: no grid is built
            res = {"keep": torch.zeros(self.points.size(0), dtype=torch.uint8, device=dev),
                   "kept": torch.zeros(S, dtype=torch.int32, device=dev), "beyond": torch.zeros(S, dtype=torch.int32, device=dev)}
        else:
            bufs = ops.scan_voxels_buffers(S, self.points.size(0), dev)
            run = lambda edge: ops.scan_voxels(self.points, self.offsets, edge.contiguous(), origin=anchor, keep=keep, out=bufs,
                                               ws=bufs["ws"])
            for _ in range(self.THIN_ROUNDS):                      # every scan at once, nothing read by the host
                mid = (lo + hi) * 0.5
                res = run(mid)
                fits = (res["kept"] <= m) & (res["beyond"] == 0)
                hi, lo = torch.where(fits, mid, hi), torch.where(fits, lo, mid)
            res = run(hi)
        whole = whole.to(dev)
        scan = self._scan_of_rows()
        present = torch.isfinite(self.points).all(1)
        mask = torch.where(whole[scan], present, res["keep"] != 0)
        rows = torch.zeros(S, dtype=torch.int64, device=dev).index_add_(0, scan, present.to(torch.int64))
        kept = torch.where(whole, rows, res["kept"].to(torch.int64))
        beyond = torch.where(whole, torch.zeros_like(rows), res["beyond"].to(torch.int64))
        kept, beyond = torch.stack([kept, beyond]).cpu()           # the host synchronisation
        bad = torch.nonzero((beyond > 0) | (kept > m))
        if bad.numel():
            s = int(bad[0])
            raise ValueError(f"scan {self._label(s)} cannot be thinned to {m} rows: {int(kept[s])} cells and {int(beyond[s])} rows "
                             f"beyond the grid at the coarsest voxel tried; {advice}")
        self.voxels = torch.where(whole, torch.full_like(hi, float("nan")), hi)
        self._keep_rows(mask, kept, f"thinning (max_points = {m})")

    def _label(self, idx):
        return f"{idx} ({self.names[idx]})" if self.names else str(idx)

    def thinned(self, voxel=None, max_points=None, keep="center", origin=None):
        """A new dataset with one row per occupied cell of a regular grid (ops.scan_voxels, csrc/voxels.hip) — the first stage
        for sensor scans: it brings a scan of hundreds of thousands of rows under the caps of without_outliers and the cluster
        methods and evens out a depth sensor's density, which a fixed cluster radius needs.  Exactly one of:
        voxel: the cell edge, a positive float (or an (S) float32 device tensor).  One ops.scan_voxels call.  A scan with
        rows beyond the grid of 2^21 cells per axis raises ValueError naming it: nothing is dropped silently.
        max_points >= 8: per scan the finest grid found by a fixed bisection that leaves at most max_points rows — 16
        rounds between 0 and the scan's box scale (ops.scan_boxes; 1 where it is 0), mid = (lo + hi) / 2 in fp32, a round is
        accepted (hi = mid) iff it keeps at most max_points rows with none beyond the grid, the edge used is the last hi; all
        scans in parallel on the device, no host synchronisation inside the loop.  Scans of at most max_points rows are left
        whole, bit for bit (rows with non-finite values go); when that is every scan, no grid is built at all.  Raises
        ValueError naming the scan the final grid does not fit.
        keep="center" keeps the row of a cell nearest its centre, keep="first" its first row: always a row of the scan, bit
        for bit, never a centroid (ops.scan_voxels' label averages per cell with one index_add_).
        origin=None anchors every grid at the coordinate origin, so a row's cell depends on its own coordinates only:
        thinning commutes with any filter that drops whole cells, and cropped and uncropped scans share cells.
        origin="center" anchors each scan's grid at its box centre (boxes()), for scans far from the origin.
        The kept rows in scan order, gt / names / scenes / obj_boxes / planes / plane_found / source_scan carried over,
        source_rows (int64, composed when the dataset was filtered before) and kept (S) set; voxels (S) float32 holds the
        edge used per scan, NaN for scans left whole.  One host synchronisation, as the other filters."""
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new._thin(voxel, max_points, keep, origin)
        return new

    def _see(self, viewpoints, keep, visibility):
        """Replaces the ragged set by the rows visible from `viewpoints` (ops.scan_visibility) and sets viewpoints.  One host
        synchronisation."""
        if keep not in ("visible", "nearest"):
            raise ValueError(f'keep must be "visible" or "nearest", got {keep!r}')
        if not self.points.is_cuda:
            raise HipExtensionError("visibility needs a dataset on the GPU — it has no CPU path")
        S, dev = len(self), self.device
        views = ops._viewpoints(viewpoints, S, dev)
        res = ops.scan_visibility(self.points, self.offsets, views, **visibility)
        mask = res["label"] == 1
        if keep == "nearest":
            mask &= res["winner"] != 0
        kept = torch.zeros(S, dtype=torch.int64, device=dev).index_add_(0, self._scan_of_rows(), mask.to(torch.int64))
        self.viewpoints = views
        self._keep_rows(mask, kept, f"the view from its sensor position (keep = {keep!r})")

    def seen_from(self, viewpoints, resolution=32, window=1, margin=0.01, slope=2.0, keep="visible"):
        """A new dataset with the rows of every scan that a sensor at `viewpoints` — one triple for all scans or (S,3), in the
        scans' frame — would record (ops.scan_visibility, csrc/visibility.hip): the near side of the object, the rest hidden
        behind it.  resolution, window, margin and slope are the law's parameters: a cube map of `resolution` pixels per
        face edge about the viewpoint, whose pixel must be about the scan's sample spacing or coarser.
        keep="visible" keeps the rows labelled on the surface, keep="nearest" of those the one row that owns its pixel: the
        even angular sampling of a range image.  The kept rows in scan order, gt / names / scenes / obj_boxes carried over,
        source_rows (int64, composed when the dataset was filtered before) and kept (S) set; viewpoints (S,3) float32 on the
        device holds the sensor positions and travels with the datasets filtered from this one (a dataset posed into another
        frame drops it).  Raises ValueError naming the scan that would be left without points.  One host synchronisation,
        as the other filters."""
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new._see(viewpoints, keep, dict(resolution=resolution, window=window, margin=margin, slope=slope))
        return new

    @classmethod
    def virtual_scans(cls, clouds, viewpoints, names=None, device=None, **visibility):
        """Self-occluded partial scans with a known answer: every complete cloud of `clouds` (S,N,3) seen from its viewpoints
        — (S,3), or (S,V,3) for V sensor positions a cloud — by seen_from(**visibility).  The result has S * V scans in
        (cloud, viewpoint) order, gt (S*V,N,3) set to the cloud each came from, names f"{name}~{v}" (name: names[s], default
        the cloud's number), source_rows the rows within the S*V repeated clouds and viewpoints (S*V,3): what ScanBatcher and
        fixed() need to score a completion of a sensor-like view against ground truth."""
        clouds = torch.as_tensor(clouds, dtype=torch.float32)
        if clouds.dim() != 3 or clouds.size(2) != 3 or clouds.size(0) < 1 or clouds.size(1) < 1:
            raise ValueError(f"clouds must be (S,N,3), got {tuple(clouds.shape)}")
        S, N = clouds.size(0), clouds.size(1)
        views = torch.as_tensor(viewpoints, dtype=torch.float32)
        if views.dim() == 2:
            views = views.unsqueeze(1)
        if views.dim() != 3 or views.size(0) != S or views.size(2) != 3 or views.size(1) < 1:
            raise ValueError(f"viewpoints must be (S,3) or (S,V,3) with S = {S}, got {tuple(views.shape)}")
        V = views.size(1)
        if names is not None and len(names) != S:
            raise ValueError("names must have one entry per cloud")
        label = [str(s) for s in range(S)] if names is None else [str(n) for n in names]
        gt = clouds.repeat_interleave(V, 0)
        whole = cls((gt.reshape(-1, 3), torch.arange(S * V + 1, dtype=torch.int64) * N), gt=gt,
                    names=[f"{label[s]}~{v}" for s in range(S) for v in range(V)], device=device)
        return whole.seen_from(views.reshape(S * V, 3), **visibility)

    def with_search(self, search):
        """The same dataset (no copy of its rows) whose neighbour searches — without_outliers, normals, without_edges — run
        by `search`: "brute" (ops.knn_points, the default of every new dataset: scans of up to ops.KNN_MAX_POINTS points) or
        "grid" (ops.knn_points_grid, csrc/knn_grid.hip: the same neighbours, rows and tensors bit for bit, scans of up to
        ops.KNN_GRID_MAX_POINTS points — a whole sensor scan, not thinned first).  The setting travels with every dataset
        filtered from this one.  Any other value is a ValueError."""
        if search not in ("brute", "grid"):
            raise ValueError(f'search must be "brute" or "grid", got {search!r}')
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new.search = search
        return new

    def without_outliers(self, k=16, ratio=2.0, search=None):
        """A new dataset without the statistical outliers of every scan (ops.scan_outliers: a row goes when its mean
        distance to its k nearest neighbours lies more than `ratio` standard deviations above the scan's average): the
        kept rows in scan order, gt / names / scenes / obj_boxes carried over, source_rows (int64, composed when the
        dataset was filtered before) and kept (S) set.  Raises ValueError naming the scan if one would be left empty or
        holds more than ops.KNN_MAX_POINTS points (nothing is subsampled silently).  One host synchronisation: this is
        still the "packed once" stage.  A cluster of at least k strays survives: they are each other's neighbours — keep_clusters
        is the remedy for those.  search: "brute" or "grid" for this call, None for the dataset's setting (with_search);
        "grid" gives the same rows by the grid-backed search (ops.scan_outliers_grid) for scans of up to
        ops.KNN_GRID_MAX_POINTS points; any other value is a ValueError."""
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new._drop_outliers(k, ratio, search)
        return new

    def normals(self, k=16, viewpoint=None):
        """(normal (T,3) float32, curvature (T) float32) of every resident row, aligned with self.points (ops.scan_normals,
        csrc/normals.hip): the unit normal of the plane through the row's k nearest neighbours and the surface variation
        lambda_min / trace of their scatter — 0 on a plane, 1/3 for an isotropic neighbourhood.  viewpoint: where the
        sensor stood, one (3,) for all scans or (S,3); every normal then faces it.  None: the normal's largest component is
        positive — a rule, not an orientation; a consistent one without a viewpoint is not built.  Rows without three
        neighbours hold NaNs.  Changes nothing in the dataset; no host synchronisation.  Raises ValueError naming the scan
        beyond ops.KNN_MAX_POINTS points: thin it first — or ask with_search("grid").normals(...): the same tensors from the
        lists of ops.knn_points_grid, for scans of up to ops.KNN_GRID_MAX_POINTS points."""
        normal, curvature, _ = self._normals(k, viewpoint, "normal estimation")
        return normal, curvature

    def without_edges(self, k=16, *, max_curvature):
        """A new dataset without the rows whose neighbourhood is far from flat (ops.scan_normals): a row stays iff its
        curvature — the surface variation over its k nearest neighbours, in [0, 1/3] — is at most max_curvature; a row
        without one (fewer than three neighbours, non-finite values) goes.  It is the filter for the mixed pixels a depth
        sensor invents between foreground and background, which without_outliers (density, not shape) leaves in; it also
        thins real creases and rims, so it belongs after without_plane and before the cluster methods.  max_curvature is
        required, 0 <= max_curvature <= 1/3: it depends on the sensor's noise and on k, read it off normals() of a clean
        patch.  The kept rows in scan order, gt / names / scenes / obj_boxes carried over, source_rows (int64, composed
        when the dataset was filtered before) and kept (S) set.  Raises ValueError naming the scan if one would be left
        empty or holds more than ops.KNN_MAX_POINTS points.  One host synchronisation, as the other filters.  On a
        with_search("grid") dataset: as normals(), scans of up to ops.KNN_GRID_MAX_POINTS points."""
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new._drop_edges(k, max_curvature)
        return new

    def without_plane(self, threshold, trials=512, seed=0, min_inliers=3, min_share=0.2, refine=True):
        """A new dataset without the dominant plane of every scan — the floor or table top that every object of a real scene
        touches and that would join them all into one component (ops.scan_plane: `trials` three-row samples per scan, the
        one with the most rows within `threshold` wins; a pure function of the rows, seed and the scan's number).  It belongs
        between without_outliers and the cluster methods, and unlike them takes scans of up to ops.SCAN_MAX_POINTS rows.
        A scan has a plane when the winner holds at least min_inliers rows and the share min_share of the scan; a scan
        without one is left whole.  refine=True refits the plane to the winner's inliers by least squares
        (ops.plane_from_moments, anchored at the sample's first row), rounds it to fp32 and drops the rows with
        |distance| <= threshold of it (ops.scan_plane_side; rows with non-finite values go with them); refine=False drops
        the winner's inliers as they are.
        The kept rows in scan order, gt / names / scenes / obj_boxes carried over, source_rows (int64, composed when the
        dataset was filtered before) and kept (S) set; planes (S,4) float32 holds each scan's unit plane (nx, ny, nz, d),
        oriented so that most of the kept rows lie on its positive side — ops.rotation_to_axis(planes[s, :3]) is the
        transform that stands the scan upright —, NaN where plane_found (S) bool is False.  Raises ValueError naming the
        scan if one would be left empty.  One host synchronisation, as the other filters; refine=True reads the moments
        (S small rows) before it.  For a second plane call it again."""
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new._drop_plane(threshold, trials, seed, min_inliers, min_share, refine)
        return new

    def keep_clusters(self, radius, min_points=None):
        """A new dataset with only the main piece of every scan (ops.scan_clusters: rows closer than `radius` are joined, the
        connected components are the pieces).  min_points None keeps each scan's largest component (equal sizes: the one
        with the smaller first row), an integer every component of at least min_points rows; rows with non-finite values
        go.  The kept rows in scan order, gt / names / scenes / obj_boxes carried over, source_rows (int64, composed when
        the dataset was filtered before) and kept (S) set.  Raises ValueError naming the scan if one would be left empty or
        holds more than ops.CLUSTER_MAX_POINTS points (nothing is subsampled silently).  One host synchronisation: this is
        still the "packed once" stage."""
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new._drop_clusters(radius, min_points)
        return new

    def split_clusters(self, radius, min_points=1):
        """A new dataset in which every connected component (ops.scan_clusters, as keep_clusters) of at least min_points rows
        is a scan of its own — scene in, objects out.  The pieces are ordered by (source scan, label), label being the
        piece's first row in its scan, and keep their rows in scan order.  source_scan (S') int64 names the scan a piece
        came from, source_rows is set (composed when the dataset was filtered before), kept is the pieces' lengths, names
        become f"{name}#{label}" when names exist, scenes / obj_boxes are carried to each piece of their scan, and gt is
        dropped: a piece has no ground truth.  Raises ValueError if no piece is left or a scan holds more than
        ops.CLUSTER_MAX_POINTS points.  One host synchronisation."""
        if int(min_points) < 1:
            raise ValueError("min_points >= 1 is required")
        label, size, _, _ = self._clusters(radius, "cluster extraction")
        rows = torch.nonzero(size >= int(min_points)).squeeze(1)   # ascending; absent rows have size 0
        key = self._scan_of_rows()[rows] * (ops.CLUSTER_MAX_POINTS + 1) + label[rows].to(torch.int64)
        key, order = torch.sort(key, stable=True)                  # by (scan, label), rows of a piece stay in scan order
        rows = rows[order]
        pieces, counts = torch.unique_consecutive(key, return_counts=True)
        pieces, counts = pieces.cpu(), counts.cpu()                # the host synchronisation
        if pieces.numel() == 0:
            raise ValueError(f"no component of at least {int(min_points)} rows at radius = {radius}")
        scan = torch.div(pieces, ops.CLUSTER_MAX_POINTS + 1, rounding_mode="floor")
        first = pieces - scan * (ops.CLUSTER_MAX_POINTS + 1)
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
        new.source_rows = rows if self.source_rows is None else self.source_rows[rows]
        new.points = self.points[rows].contiguous()
        new.offsets, new.offsets_host = offsets.to(self.device).contiguous(), offsets
        new.lengths = new.kept = counts
        new._boxes = None
        new.source_scan = scan if self.source_scan is None else self.source_scan[scan]
        if self.planes is not None:
            new.planes, new.plane_found = self.planes[scan.to(self.device)], self.plane_found[scan.to(self.device)]
        if self.voxels is not None:
            new.voxels = self.voxels[scan.to(self.device)]
        if self.viewpoints is not None:
            new.viewpoints = self.viewpoints[scan.to(self.device)]
        new.gt = None
        new.pixels = new.pixel_normals = None                      # the pieces' rows are reordered: the lineage ends here
        carry = lambda seq: None if seq is None else [seq[int(i)] for i in scan]
        new.scenes, new.obj_boxes = carry(self.scenes), carry(self.obj_boxes)
        if self.names is not None:
            new.names = [f"{self.names[int(i)]}#{int(l)}" for i, l in zip(scan, first)]
        return new

    def _check_align(self, lengths, what, label):
        """The checks of an alignment the host can make: the device, and the cap of ops.scan_align_step on `lengths`."""
        if not self.points.is_cuda:
            raise HipExtensionError(f"{what} needs a dataset on the GPU — it has no CPU path")
        longest = int(lengths.argmax())
        if int(lengths[longest]) > ops.ALIGN_MAX_POINTS:
            raise ValueError(f"{label(longest)} holds {int(lengths[longest])} points: {what} takes sets of at most "
                             f"{ops.ALIGN_MAX_POINTS} points (brute-force matching, exact 64-bit sums) and does not "
                             f"subsample; thin it first")

    @staticmethod
    def _moved(points, offsets, poses, ok):
        """The rows under their set's pose, p' = R p + t in fp32; the rows of a set that is not ok stay bit for bit."""
        lengths = (offsets[1:] - offsets[:-1])
        rows = torch.repeat_interleave(torch.arange(len(ok), device=points.device), lengths, output_size=points.size(0))
        m = torch.from_numpy(poses.astype(np.float32)).to(points.device)[rows]
        moved = (m[:, :, :3] * points.unsqueeze(1)).sum(2) + m[:, :, 3]
        moved = torch.where(torch.from_numpy(ok).to(points.device)[rows].unsqueeze(1), moved, points)
        return moved.contiguous()

    def _posed(self, points, offsets, tpoints, toffsets, max_dist, iters, yaw, axis):
        """(posed points, poses (S,3,4) float64, ok, rms) of ops.scan_align over the given sets: a set that does not align
        keeps its rows bit for bit and the identity as its pose."""
        poses, ok, rms, _, _ = ops.scan_align(points, offsets, tpoints, toffsets, max_dist, iters=iters, yaw=yaw, axis=axis)
        poses[~ok, :, :3], poses[~ok, :, 3] = np.eye(3), 0.0
        return self._moved(points, offsets, poses, ok), poses, ok, rms

    def _posed_surface(self, points, offsets, tpoints, toffsets, max_dist, iters, yaw, axis, k, coarse):
        """(posed points, poses, ok, rms) of the two-stage alignment: `coarse` steps of ops.scan_align (with its yaw search),
        then ops.scan_align_plane from those poses.  A set whose refinement is not ok keeps its coarse pose where that was
        ok, otherwise its rows bit for bit and the identity; ok is true where either stage was.  rms is the point-to-plane
        rms of the refinement's last step."""
        S = len(offsets) - 1
        start, start_ok = np.tile(np.eye(3, 4), (S, 1, 1)), np.zeros(S, dtype=bool)
        if int(coarse) > 0 or int(yaw) > 0:
            start, start_ok, _, _, _ = ops.scan_align(points, offsets, tpoints, toffsets, max_dist, iters=coarse, yaw=yaw, axis=axis)
            start[~start_ok, :, :3], start[~start_ok, :, 3] = np.eye(3), 0.0
        poses, fine_ok, rms, _ = ops.scan_align_plane(points, offsets, tpoints, toffsets, max_dist, iters=iters, init=start, k=k)
        poses[~fine_ok] = start[~fine_ok]
        ok = fine_ok | start_ok
        return self._moved(points, offsets, poses, ok), poses, ok, rms

    def aligned_to(self, targets, max_dist, iters=30, yaw=0, axis=(0, 1, 0)):
        """A new dataset whose scans are posed onto `targets` by point-to-point ICP (ops.scan_align, csrc/align.hip) — the
        last stage before ScanBatcher: a cleaned scan against a template, a ground truth or another dataset's scans.
        targets: one (m,3) cloud for all scans, a list of S clouds, a (points, offsets) pair, or a DeviceScanDataset of S
        scans.  max_dist gates the correspondences (+inf: none); yaw = H > 0 starts from H turns about `axis` through the box
        centres and keeps each scan's best (the remedy for an arbitrary angle about the up axis); iters refinement steps.
        The posed rows in scan order, p' = R p + t in fp32; poses (S,3,4) float64 scan -> target, pose_ok (S) bool and
        pose_rms (S) float64 as numpy arrays; gt / names / scenes / obj_boxes / planes / voxels / source_rows / kept /
        source_scan pass through unchanged (planes and gt stay in the old frame).  A scan that does not align — fewer than
        three correspondences, or all on a line — stays as it was, with the identity pose and pose_ok False.  Raises
        ValueError naming the scan or target beyond ops.ALIGN_MAX_POINTS points: thin it first.  The host reads the moments
        (144 bytes a scan) once per iteration, as without_plane does for its refit."""
        return self._aligned(targets, lambda *sets: self._posed(*sets, max_dist, iters, yaw, axis))

    def _aligned(self, targets, pose):
        """aligned_to and aligned_to_surface: the targets in their forms, the checks, and the new dataset; pose(points,
        offsets, tpoints, toffsets) -> (posed points, poses, ok, rms) is the aligner."""
        S = len(self)
        if isinstance(targets, DeviceScanDataset):
            tpoints, toffsets = targets.points, targets.offsets_host
        elif isinstance(targets, tuple) or (isinstance(targets, list) and len(targets) and torch.as_tensor(targets[0]).dim() == 2):
            tpoints, toffsets = _pack(targets)
        else:
            one = torch.as_tensor(targets)
            if one.dim() != 2 or one.size(1) != 3 or one.size(0) < 1:
                raise ValueError(f"targets must be an (m,3) cloud or one cloud per scan, got {tuple(one.shape)}")
            tpoints, toffsets = one.to(torch.float32), None
        tlengths = torch.tensor([tpoints.size(0)]) if toffsets is None else (toffsets[1:] - toffsets[:-1]).cpu()
        if toffsets is not None and tlengths.numel() != S:
            raise ValueError(f"targets must hold one cloud per scan: {tlengths.numel()} for {S} scans")
        self._check_align(self.lengths, "alignment", lambda i: f"scan {self._label(i)}")
        self._check_align(tlengths, "alignment", lambda i: f"target {i}")
        dev = self.device
        tpoints = tpoints.to(dev).contiguous()
        if toffsets is None:                                       # one cloud for all: S sets over the same rows
            tpoints = tpoints.repeat(S, 1)
            toffsets = torch.arange(S + 1, dtype=torch.int64) * int(tlengths[0])
        toffsets = toffsets.to(dev).contiguous()
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new.points, new.poses, new.pose_ok, new.pose_rms = pose(self.points, self.offsets, tpoints, toffsets)
        new._boxes = None
        new.viewpoints = None                                      # the sensor stood in the old frame
        new.pixels = new.pixel_normals = None                      # ... and the images' normals point in it
        return new

    def aligned_to_surface(self, targets, max_dist, iters=10, yaw=0, axis=(0, 1, 0), k=16, coarse=5):
        """aligned_to with the point-to-plane error (ops.scan_align_plane, csrc/align_plane.hip) — the aligner for surfaces: a
        depth sensor's two captures never sample the same points, point-to-point ICP pulls every row to its nearest sample
        and the pose crawls along the surface; the distance along the target's normal does not.  targets, max_dist, yaw and
        axis as aligned_to.  Two stages: `coarse` point-to-point steps (ops.scan_align, with the yaw search when yaw > 0;
        coarse = 0 with yaw = 0 skips the stage) bring the scan within reach, then `iters` point-to-plane steps from those
        poses refine it, on the targets' normals over k neighbours (ops.scan_normals, computed once).  poses, pose_ok and
        pose_rms as aligned_to; pose_rms is the rms point-to-plane distance of the refinement's last step.  A scan whose
        refinement is refused — fewer than six correspondences with a normal, or a target that lets the scan slide, as one
        plane does — keeps its coarse pose if that was ok (pose_ok True), otherwise its rows and the identity (pose_ok
        False).  Raises as aligned_to."""
        return self._aligned(targets, lambda *sets: self._posed_surface(*sets, max_dist, iters, yaw, axis, k, coarse))

    def merged_views(self, groups, max_dist, iters=30, yaw=0, axis=(0, 1, 0)):
        """A new dataset with one scan per group of views: every scan of a group is aligned to the group's first scan
        (ops.scan_align, as aligned_to) and the posed rows are concatenated in group order — two or three captures of one
        object in one frame, the union a completion model wants as its input.  groups: a list of lists of scan numbers.
        source_scan (G) int64 is the first scan of each group (composed when the dataset was split before), view_rows a list
        of G lists: the rows each view contributed; poses, pose_ok, pose_rms are lists of G arrays, one entry per view (the
        first view has the identity, True and 0); a view that does not align is merged as it was, pose_ok False.  names / scenes /
        obj_boxes / planes / voxels / gt are carried from each group's first scan; source_rows and kept are dropped (a
        merged row has no single origin).  Raises ValueError naming the group whose merged scan would exceed
        ops.SCAN_MAX_POINTS rows, or whose scan exceeds ops.ALIGN_MAX_POINTS: thin first."""
        return self._merged(groups, lambda *sets: self._posed(*sets, max_dist, iters, yaw, axis))

    def merged_views_surface(self, groups, max_dist, iters=10, yaw=0, axis=(0, 1, 0), k=16, coarse=5):
        """merged_views with aligned_to_surface's aligner: every further view of a group is posed onto the group's first view
        by `coarse` point-to-point steps and `iters` point-to-plane steps on that view's normals.  Everything else —
        groups, source_scan, view_rows, the lists poses / pose_ok / pose_rms, what is carried and what raises — as
        merged_views; a view whose refinement is refused keeps its coarse pose, as in aligned_to_surface."""
        return self._merged(groups, lambda *sets: self._posed_surface(*sets, max_dist, iters, yaw, axis, k, coarse))

    def _posed_globally(self, points, offsets, tpoints, toffsets, max_dist, iters, k, trials, seed, viewpoint, target_viewpoint,
                        surface, coarse, found):
        """(posed points, poses, ok, rms) of the alignment from a global start: ops.scan_align_global, then `coarse` steps of
        ops.scan_align from its poses (`iters` without surface) and, with surface, ops.scan_align_plane from those.  A set that
        a stage refuses keeps the stage before; ok is true where any stage, the global start included, was.  `found` (a list)
        receives the global start's found (S) bool."""
        view = lambda v: None if v is None else torch.as_tensor(v, dtype=torch.float32).to(points.device).contiguous()
        start, start_ok, _, _ = ops.scan_align_global(points, offsets, tpoints, toffsets, max_dist, k=k, trials=trials, seed=seed,
                                                      viewpoints=view(viewpoint),
                                                      tviewpoints=view(viewpoint if target_viewpoint is None else target_viewpoint))
        found.append(start_ok)
        poses, ok, rms, _, _ = ops.scan_align(points, offsets, tpoints, toffsets, max_dist, iters=coarse if surface else iters,
                                              init=start)
        poses[~ok] = start[~ok]
        ok = ok | start_ok
        if surface:
            fine, fine_ok, rms, _ = ops.scan_align_plane(points, offsets, tpoints, toffsets, max_dist, iters=iters, init=poses, k=k)
            poses[fine_ok] = fine[fine_ok]
            ok = ok | fine_ok
        return self._moved(points, offsets, poses, ok), poses, ok, rms

    def aligned_globally(self, targets, max_dist, iters=10, k=32, trials=32768, seed=0, viewpoint=(0, 0, 0), target_viewpoint=None,
                         surface=True, coarse=5):
        """aligned_to_surface from a global start (ops.scan_align_global: descriptors over k neighbours, their nearest
        matches, `trials` matched triples, csrc/features.hip and csrc/pose_trials.hip) — for a scan in an arbitrary pose
        against its target: a hand-held capture, a view turned about any axis, a completion in a frame of its own.  The
        local aligners only converge from a close pose, and yaw covers one known axis.  targets and max_dist as aligned_to;
        max_dist is also the inlier distance of the consensus.  viewpoint: where the sensor of the scans stood, in their
        frame, one (3,) or (S,3) — the normals face it, and descriptors need that; target_viewpoint: the same for the
        targets, default viewpoint.  From the start found, `coarse` point-to-point steps and, with surface, `iters`
        point-to-plane steps (without surface: `iters` point-to-point steps).  A scan without a start takes that path from
        the identity.  poses, pose_ok, pose_rms as aligned_to_surface, and pose_found (S) bool: the global start was found."""
        found = []
        new = self._aligned(targets, lambda *sets: self._posed_globally(*sets, max_dist, iters, k, trials, seed, viewpoint,
                                                                         target_viewpoint, surface, coarse, found))
        new.pose_found = found[0]
        return new

    def merged_views_globally(self, groups, max_dist, iters=10, k=32, trials=32768, seed=0, surface=True, coarse=5):
        """merged_views_surface with aligned_globally's aligner: every further view of a group is posed onto the group's first
        view from a global start, whatever their relative pose.  Each view is oriented to its own origin: a capture's rows are
        in its sensor's frame.  Everything else as merged_views; pose_found is a list of G arrays, one entry per view (True
        for a group's first view)."""
        found = []
        new = self._merged(groups, lambda *sets: self._posed_globally(*sets, max_dist, iters, k, trials, seed, (0, 0, 0), None,
                                                                      surface, coarse, found))
        flags = np.ones(sum(len(g) for g in groups), dtype=bool)
        cut = np.cumsum([0] + [len(g) for g in groups])
        if found:
            lead = np.zeros(len(flags), dtype=bool)
            lead[cut[:-1]] = True
            flags[~lead] = found[0]
        new.pose_found = [flags[cut[i]:cut[i + 1]] for i in range(len(groups))]
        return new

    def _merged(self, groups, pose):
        """merged_views and merged_views_surface: the checks, the gathering of the views and the concatenation; pose(points,
        offsets, tpoints, toffsets) -> (posed points, poses, ok, rms) is the aligner."""
        groups = [[int(i) for i in g] for g in groups]
        S = len(self)
        if not groups or any(not g for g in groups) or any(not 0 <= i < S for g in groups for i in g):
            raise ValueError(f"groups must be non-empty lists of scan numbers in [0, {S})")
        for k, g in enumerate(groups):
            total = sum(int(self.lengths[i]) for i in g)
            if total > ops.SCAN_MAX_POINTS:
                raise ValueError(f"group {k} would merge into {total} points: a scan holds at most {ops.SCAN_MAX_POINTS}; thin first")
        pairs = [(k, i) for k, g in enumerate(groups) for i in g]  # the views in merged order
        views = torch.tensor([i for _, i in pairs], dtype=torch.int64)
        self._check_align(self.lengths[views], "merging views",
                          lambda j: f"scan {self._label(pairs[j][1])} of group {pairs[j][0]}")
        dev = self.device

        def gather(ids):
            lengths = self.lengths[ids]
            offsets = torch.cat([torch.zeros(1, dtype=torch.int64), lengths.cumsum(0)])
            start = self.offsets_host[:-1][ids]
            rows = torch.repeat_interleave(start - offsets[:-1], lengths) + torch.arange(int(offsets[-1]))
            return self.points[rows.to(dev)].contiguous(), offsets

        points, offsets = gather(views)
        cut = np.cumsum([0] + [len(g) for g in groups])
        lead = np.zeros(len(pairs), dtype=bool)
        lead[cut[:-1]] = True                                      # a group's first view is the frame itself: kept bit for bit
        poses = np.tile(np.eye(3, 4), (len(pairs), 1, 1))
        ok, rms = np.ones(len(pairs), dtype=bool), np.zeros(len(pairs), dtype=np.float64)
        if not lead.all():                                         # one set per further view, against its group's first view
            rest = torch.from_numpy(~lead)
            firsts = torch.tensor([groups[k][0] for k, _ in pairs], dtype=torch.int64)[rest]
            sources, soffsets = gather(views[rest])
            tpoints, toffsets = gather(firsts)
            moved, poses[~lead], ok[~lead], rms[~lead] = pose(sources, soffsets.to(dev), tpoints, toffsets.to(dev))
            points[torch.repeat_interleave(rest, offsets[1:] - offsets[:-1]).to(dev)] = moved      # a copy of its own: gather made it
        counts = torch.tensor([sum(int(self.lengths[i]) for i in g) for g in groups], dtype=torch.int64)
        merged = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new.points = points
        new.offsets, new.offsets_host = merged.to(dev).contiguous(), merged
        new.lengths = counts
        new._boxes = None
        new.source_rows = new.kept = None
        new.pixels = new.pixel_normals = None                      # rows of several views: no lineage to the images
        first = torch.tensor([g[0] for g in groups], dtype=torch.int64)
        new.source_scan = first if self.source_scan is None else self.source_scan[first]
        new.view_rows = [[int(self.lengths[i]) for i in g] for g in groups]
        new.poses = [poses[cut[k]:cut[k + 1]] for k in range(len(groups))]
        new.pose_ok = [ok[cut[k]:cut[k + 1]] for k in range(len(groups))]
        new.pose_rms = [rms[cut[k]:cut[k + 1]] for k in range(len(groups))]
        carry = lambda seq: None if seq is None else [seq[int(i)] for i in first]
        new.names, new.scenes, new.obj_boxes = carry(self.names), carry(self.scenes), carry(self.obj_boxes)
        for name in ("gt", "planes", "plane_found", "voxels", "viewpoints"):
            t = getattr(self, name)
            setattr(new, name, None if t is None else t[first.to(t.device)])
        return new

    @classmethod
    def from_npy_dir(cls, root, device=None, transform=None, outliers=None, clusters=None, plane=None):
        """A directory in the real-scan layout (datasets/real_data.py:18-24): files that start with `object_box` are boxes,
        other `object*` files the scans, `scen*` files the scenes; each role in sorted order, so the i-th of each belong
        together.  outliers=(k, ratio), clusters=(radius, min_points), plane=(threshold, trials): as in the constructor."""
        roles = {"obj_boxes": [], "scans": [], "scenes": []}
        for f in sorted(os.listdir(root)):
            if f.startswith("object_box"):
                roles["obj_boxes"].append(f)
            elif f.startswith("object"):
                roles["scans"].append(f)
            elif f.startswith("scen"):
                roles["scenes"].append(f)
        if not roles["scans"]:
            raise ValueError(f"{root}: no object*.npy scans")
        read = lambda names: [np.load(os.path.join(root, n)).astype(np.float32) for n in names]
        return cls(read(roles["scans"]), names=roles["scans"], transform=transform, device=device,
                   scenes=read(roles["scenes"]) or None, obj_boxes=read(roles["obj_boxes"]) or None, outliers=outliers,
                   clusters=clusters, plane=plane)

    @classmethod
    def from_depth_images(cls, depth, intrinsics, poses=None, masks=None, depth_scale=None, near=0.0, far=float("inf"),
                          jump=(0.0, 0.05), window=1, names=None, device=None):
        """What a depth sensor delivers, as a dataset (ops.depth_points, csrc/depth.hip): depth (B,H,W) uint16 or float32,
        intrinsics (4,) or (B,4) = (fx, fy, cx, cy), poses camera-to-world ((3,4), (B,3,4) or 4x4; None: the camera frame),
        masks (B,H,W) uint8 or None, and depth_scale, near, far, jump, window as ops.depth_points — arrays or tensors, uploaded
        once; intrinsics and poses are host data, checked there.  Every image becomes a scan in the world frame: its pixels that are measured, in range, masked in and not at a
        depth edge, in row, column order — no holes, no mixed pixels, nothing to convert by hand.  points, offsets and
        lengths are trimmed to the kept rows; viewpoints (B,3) holds each pose's translation, where the sensor stood, and
        travels as it does after seen_from; pixels (T) int64 = (b * H + v) * W + u and pixel_normals (T,3) float32 (unit,
        facing the sensor, from the pixel grid; zero where a pixel has no usable neighbour pair) are aligned with the rows as
        built: row_pixels() and row_normals() give them for the current rows of any dataset filtered from this one.
        search is "grid" when some image keeps more than ops.KNN_MAX_POINTS rows — a whole sensor image is beyond the
        brute-force searches — and "brute" otherwise (with_search changes it).  An image that keeps no pixel is a ValueError
        naming it.  One host synchronisation, reading the offsets, as the other constructors."""
        if device is None:
            device = depth.device if torch.is_tensor(depth) and depth.is_cuda else torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        depth = torch.as_tensor(depth).to(device).contiguous()
        if masks is not None:
            masks = torch.as_tensor(masks).to(device).contiguous()
        if depth.dim() != 3:
            raise ValueError(f"depth must be (B,H,W), got {tuple(depth.shape)}")
        B = depth.size(0)
        names = None if names is None else [str(n) for n in names]
        if names is not None and len(names) != B:
            raise ValueError("names must have one entry per image")
        K, M = ops.depth_points_tables(B, intrinsics, poses, device)       # checked on the host, uploaded once
        res = ops.depth_points(depth, K, poses=M, masks=masks, depth_scale=depth_scale, near=near, far=far, jump=jump, window=window)
        offsets = res["offsets"].cpu()                             # the host synchronisation
        lengths = offsets[1:] - offsets[:-1]
        empty = torch.nonzero(lengths == 0)
        if empty.numel():
            i = int(empty[0])
            raise ValueError(f"image {f'{i} ({names[i]})' if names else i} keeps no pixel: nothing measured, in range, masked in "
                             f"and off the depth edges")
        T = int(offsets[-1])
        new = object.__new__(cls)                                  # the attributes of __init__, stated for rows that are on the device already
        new.points = res["points"][:T].contiguous()
        new.offsets, new.offsets_host, new.lengths = res["offsets"], offsets, lengths
        new.gt, new.names, new.scenes, new.obj_boxes, new._boxes = None, names, None, None, None
        new.source_rows = new.kept = new.source_scan = None
        new.planes = new.plane_found = new.voxels = None
        new.poses = new.pose_ok = new.pose_rms = new.view_rows = None
        new.search = "grid" if int(lengths.max()) > ops.KNN_MAX_POINTS else "brute"
        new.viewpoints = M[:, :, 3].contiguous()
        new.pixels, new.pixel_normals = res["pixel"][:T].contiguous(), res["normals"][:T].contiguous()
        new.volume = None
        return new

    @classmethod
    def fused_depth_images(cls, depth, intrinsics, poses, groups=None, voxel=None, truncation=None, bounds=None, min_weight=1,
                           masks=None, depth_scale=None, near=0.0, far=float("inf"), jump=(0.0, 0.05), window=1, names=None,
                           device=None):
        """Several posed depth images of one surface, fused (ops.fuse_volume and ops.fuse_surface, csrc/fuse.hip): one scan
        per group of images, in the world frame.  Where from_depth_images makes a scan of every image and merged_views*
        registers and concatenates them, this averages the images in a truncated signed distance volume of `voxel`-sized
        cells: depth noise is averaged, overlap is sampled once, and what one image records where the others look straight
        through — a flying pixel, a stray blob — is carved away.  depth, intrinsics, poses, masks, depth_scale, near, far,
        jump, window as from_depth_images, poses required; groups: a list of lists of image numbers (None: all images, one
        scan); voxel: required; truncation: None for 4 * voxel; bounds: (lo, hi), each (3,) or (G,3), the boxes to fuse within
        — None: the bounding box of each group's kept back-projected points (ops.depth_points, reduced on the device, one
        host read), grown by ops.fuse_grid.  min_weight: the images that must observe a voxel for it to carry surface.
        pixel_normals holds the fused normals (unit, into free space), so row_normals() follows them through the filters;
        pixels and viewpoints are None: row_pixels() raises, as after merged_views*.  volume keeps the fuse_volume result.
        A group without a row, or with more than ops.SCAN_MAX_POINTS, is a ValueError naming it."""
        if voxel is None:
            raise ValueError("voxel, the edge of a volume's cells, is required")
        if device is None:
            device = depth.device if torch.is_tensor(depth) and depth.is_cuda else torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        depth = torch.as_tensor(depth).to(device).contiguous()
        if masks is not None:
            masks = torch.as_tensor(masks).to(device).contiguous()
        if depth.dim() != 3:
            raise ValueError(f"depth must be (B,H,W), got {tuple(depth.shape)}")
        if poses is None:
            raise ValueError("poses are required: fusion brings the images into one frame")
        B = depth.size(0)
        images, ends = ops._fuse_groups(groups, B)
        G = ends.numel() - 1
        names = None if names is None else [str(n) for n in names]
        if names is not None and len(names) != G:
            raise ValueError("names must have one entry per group")
        label = lambda g: f"{g} ({names[g]})" if names else str(g)
        voxel, truncation = ops._check_fuse_lengths(voxel, truncation)
        K, M = ops._depth_intrinsics(intrinsics, B), ops._depth_poses(poses, B)        # checked on the host, uploaded once
        ops._check_rotations(M)
        K, M = K.to(device), M.to(device)
        kw = dict(masks=masks, depth_scale=depth_scale, near=near, far=far, jump=jump, window=window)
        if bounds is None:
            res = ops.depth_points(depth, K, poses=M, **kw)
            big = torch.finfo(torch.float32).max
            first, last = res["offsets"][images.to(device).long()], res["offsets"][images.to(device).long() + 1]
            rows = torch.arange(res["points"].size(0), device=device)
            box = []
            for g in range(G):                                         # per group: its images' rows, wherever they lie
                a, b = int(ends[g]), int(ends[g + 1])
                mine = ((rows[None, :] >= first[a:b, None]) & (rows[None, :] < last[a:b, None])).any(0)[:, None]
                box.append(torch.cat([torch.where(mine, res["points"], big).amin(0), torch.where(mine, res["points"], -big).amax(0)]))
            box = torch.stack(box).cpu().to(torch.float64)             # the host read
            for g in range(G):
                if not bool((box[g, :3] <= box[g, 3:]).all()):
                    raise ValueError(f"group {label(g)} keeps no pixel: nothing measured, in range, masked in and off the depth edges")
            lo, hi = box[:, :3], box[:, 3:]
        else:
            try:
                lo, hi = (ops._depth_table(x, G, (3,), "bounds", "(lo, hi), each (3,) or (G,3)") for x in bounds)
            except TypeError:
                raise ValueError("bounds must be a pair (lo, hi)") from None
        origin, dims = ops.fuse_grid(lo, hi, voxel, truncation)
        volume = ops.fuse_volume(depth, K, M, [images[int(ends[g]):int(ends[g + 1])].tolist() for g in range(G)], origin, dims, voxel,
                                 truncation, **kw)
        res = ops.fuse_surface(volume, min_weight=min_weight)          # the host synchronisation: the rows are counted, then emitted
        offsets = res["offsets"].cpu()
        lengths = offsets[1:] - offsets[:-1]
        for g in range(G):
            if int(lengths[g]) == 0:
                raise ValueError(f"group {label(g)} has no surface: no two neighbouring voxels observed {min_weight} times lie on "
                                 f"either side of one")
            if int(lengths[g]) > ops.SCAN_MAX_POINTS:
                raise ValueError(f"group {label(g)} has {int(lengths[g])} rows, more than {ops.SCAN_MAX_POINTS}: choose a larger voxel")
        new = object.__new__(cls)                                  # the attributes of __init__, stated for rows that are on the device already
        new.points = res["points"]
        new.offsets, new.offsets_host, new.lengths = res["offsets"], offsets, lengths
        new.gt, new.names, new.scenes, new.obj_boxes, new._boxes = None, names, None, None, None
        new.source_rows = new.kept = new.source_scan = None
        new.planes = new.plane_found = new.voxels = None
        new.poses = new.pose_ok = new.pose_rms = new.view_rows = None
        new.search = "grid" if int(lengths.max()) > ops.KNN_MAX_POINTS else "brute"
        new.viewpoints = None
        new.pixels, new.pixel_normals = None, res["normals"]
        new.volume = volume
        return new

    def _of_images(self, what, name):
        if what is None:
            raise ValueError(f"{name} needs the rows' lineage to depth images: the dataset was not made by from_depth_images, or "
                             f"an operation since (split_clusters, merged_views*, aligned_*) broke it")
        return what if self.source_rows is None else what[self.source_rows]

    def row_pixels(self):
        """(T) int64: the pixel (b * H + v) * W + u every current row was measured at — pixels of from_depth_images, followed
        through the filters by source_rows.  Raises ValueError on a dataset that did not come from depth images, and after
        split_clusters, merged_views* and aligned_*, which break the rows' lineage."""
        return self._of_images(self.pixels, "row_pixels")

    def row_normals(self):
        """(T,3) float32: the pixel-grid normal of every current row (pixel_normals of from_depth_images), in the world frame,
        facing the sensor.  Raises as row_pixels."""
        return self._of_images(self.pixel_normals, "row_normals")

    def __len__(self):
        return self.lengths.numel()

    @property
    def device(self):
        return self.points.device

    def scan(self, idx):
        """Scan idx as an (n,3) view of the resident points."""
        return self.points[int(self.offsets_host[idx]):int(self.offsets_host[idx + 1])]

    def boxes(self):
        """(center (S,3), scale (S)) of the scans (ops.scan_boxes), computed at the first call."""
        if self._boxes is None:
            self._boxes = ops.scan_boxes(self.points, self.offsets)
        return self._boxes

    def get_scene(self, idx):
        if not self.scenes:
            raise ValueError("the dataset holds no scenes")
        return torch.as_tensor(self.scenes[idx], dtype=torch.float32).to(self.device)

    def get_obj_box(self, idx):
        if not self.obj_boxes:
            raise ValueError("the dataset holds no object boxes")
        return torch.as_tensor(self.obj_boxes[idx], dtype=torch.float32).to(self.device)

    def inverse_scale(self, idx, completions):
        """Completions (N,3) or (K,N,3) of the normalised scan idx, back in the scan's coordinates: each divided by its own
        box scale, times the scan's, plus the scan's center (datasets/real_data.py:63-67)."""
        c = completions.to(self.device, torch.float32)
        single = c.dim() == 2
        c = (c.unsqueeze(0) if single else c).contiguous()
        K, N = c.size(0), c.size(1)
        own = ops.scan_boxes(c.view(-1, 3), torch.arange(K + 1, dtype=torch.int64, device=self.device) * N)[1]
        center, scale = self.boxes()
        out = ops.restore_scans(c, own, center[idx], scale[idx])
        return out[0] if single else out

    def inverse_scale_to_scene(self, idx, completions):
        """The scene of scan idx followed by inverse_scale(idx, completions): (Ns + N, 3), or (K, Ns + N, 3) for K."""
        scene = self.get_scene(idx)
        restored = self.inverse_scale(idx, completions)
        if restored.dim() == 2:
            return torch.cat([scene, restored])
        return torch.cat([scene.unsqueeze(0).expand(restored.size(0), -1, -1), restored], 1)


class ScanBatcher:
    """Iterating yields (existing (B,target,3), ids (B) int32, gt (B,N,3) or None) device tensors over every (scan, draw),
    draw < draws, in that order.  Stream id = scan * draws + draw: a scan is resampled identically in every run and whatever
    the batch size.  normalize=True maps every scan into its bounding box, (p - center) / scale.  Buffers are allocated once
    (a batch is valid until the next `next()`), nothing synchronises with the host; failures() reads the counter on demand.

    resample="subset" brings a scan to `target` rows by ops.prepare_scans' law (a keyed uniform subset when it is long).
    resample="farthest" makes a batch in two stages: prepare_scans (replace=False, same seed, streams and normalisation) to
    pool_eff = max(target, min(pool, SCAN_MAX_TARGET)) rows, then ops.farthest_points over the first min(n, pool_eff) of
    them from row 0 and a gather.  So a scan of n <= pool points is sampled by exact farthest-point sampling over all of
    them (stage 1 is the identity on its first n rows; with n < target the tail repeats row 0), a longer one by
    farthest-point sampling over a keyed uniform subset of `pool` points, and draws > 1 differ only for scans with n > pool.
    The lengths come from dataset.lengths once, here: still no synchronisation per batch.

    After each `next()`, last_index (B,target) int32 holds the scan rows of the batch (under "farthest" the pool's rows
    composed with the picks) and, under "farthest", last_radius2 (B) the squared covering radius of the kept points over
    the pool (None under "subset"): views of buffers allocated once, valid until the next `next()`."""

    def __init__(self, dataset, batch_size, target=1024, normalize=False, replace=False, seed=0, draws=1, resample="subset",
                 pool=8192):
        if not isinstance(dataset, DeviceScanDataset):
            raise TypeError("dataset must be a DeviceScanDataset")
        if resample not in ("subset", "farthest"):
            raise ValueError(f'resample must be "subset" or "farthest", got {resample!r}')
        if resample == "farthest" and replace:
            raise ValueError('replace=True has no meaning with resample="farthest": the pool is a subset without replacement')
        if resample == "farthest" and int(pool) < 1:
            raise ValueError("pool >= 1 is required")
        if not dataset.points.is_cuda:
            raise HipExtensionError("ScanBatcher needs a dataset on the GPU — scan preparation has no CPU path")
        if batch_size < 1 or draws < 1 or not (1 <= target <= ops.SCAN_MAX_TARGET):
            raise ValueError(f"batch_size >= 1, draws >= 1 and 1 <= target <= {ops.SCAN_MAX_TARGET} are required")
        self.dataset, self.batch_size, self.target = dataset, int(batch_size), int(target)
        self.normalize, self.replace, self.seed, self.draws = bool(normalize), bool(replace), int(seed), int(draws)
        self.resample = resample
        dev = dataset.device
        self._center = self._scale = None
        if self.normalize:
            self._center, self._scale = dataset.boxes()
            if bool((self._scale == 0).any()):                     # once, at construction
                raise ValueError("normalize=True needs scans of non-zero extent")
        items = torch.arange(len(dataset) * self.draws, dtype=torch.int64, device=dev)
        self._streams = items.contiguous()
        self._ids = torch.div(items, self.draws, rounding_mode="floor").to(torch.int32).contiguous()
        self._failed = torch.zeros((1,), dtype=torch.int32, device=dev)
        self._bufs = ops.prepare_scans_buffers(self.batch_size, self.target, dev)
        self._gt = None if dataset.gt is None else torch.empty((self.batch_size,) + tuple(dataset.gt.shape[1:]),
                                                              dtype=torch.float32, device=dev)
        self.last_index = self.last_radius2 = self.pool = None
        if resample == "farthest":
            self.pool = max(self.target, min(int(pool), ops.SCAN_MAX_TARGET))
            self._pool_bufs = ops.prepare_scans_buffers(self.batch_size, self.pool, dev)
            self._fps_bufs = ops.farthest_points_buffers(self.batch_size, self.target, dev)
            self._picks = torch.empty((self.batch_size, self.target), dtype=torch.int64, device=dev)
            counts = dataset.lengths.clamp(max=self.pool).to(torch.int32).repeat_interleave(self.draws)
            self._counts = counts.to(dev).contiguous()             # per item, from the host's lengths: no synchronisation later

    def __len__(self):
        return -(-self._ids.numel() // self.batch_size)

    def failures(self):
        """Items so far that were served as zeros (a scan id out of range) or, under resample="farthest", without picks."""
        return int(self._failed.item())

    def _farthest(self, lo, hi, ids, bufs):
        """One batch of resample="farthest" into bufs: the pool, the picks, then the picked rows and their scan rows."""
        data, n = self.dataset, hi - lo
        cut = (lambda d: d) if n == self.batch_size else (lambda d: {name: t[:n] for name, t in d.items()})
        pool, pool_index, _ = ops.prepare_scans(data.points, data.offsets, ids, self._streams[lo:hi], self.pool, False, self.seed,
                                                self._center, self._scale, out=cut(self._pool_bufs), failed=self._failed)
        fps = cut(self._fps_bufs)
        ops.farthest_points(pool, self.target, counts=self._counts[lo:hi], out=fps, failed=self._failed)
        picks = self._picks[:n].copy_(fps["index"]).clamp_(min=0)  # an item without picks (-1, counted) is served as row 0
        torch.gather(pool, 1, picks.unsqueeze(-1).expand(-1, -1, 3), out=bufs["existing"])
        torch.gather(pool_index, 1, picks, out=bufs["index"])
        self.last_radius2 = fps["radius2"][:, self.target - 1]
        return bufs["existing"]

    def __iter__(self):
        data = self.dataset
        for k in range(len(self)):
            lo, hi = k * self.batch_size, min((k + 1) * self.batch_size, self._ids.numel())
            bufs = self._bufs if hi - lo == self.batch_size else {n: t[:hi - lo] for n, t in self._bufs.items()}
            ids = self._ids[lo:hi]
            if self.resample == "farthest":
                existing = self._farthest(lo, hi, ids, bufs)
            else:
                existing, _, _ = ops.prepare_scans(data.points, data.offsets, ids, self._streams[lo:hi], self.target, self.replace,
                                                   self.seed, self._center, self._scale, out=bufs, failed=self._failed)
            self.last_index = bufs["index"]
            gt = None
            if self._gt is not None:
                gt = torch.index_select(data.gt, 0, ids.long(), out=self._gt[:hi - lo])
            yield existing, ids, gt
