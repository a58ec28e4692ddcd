"""Training data that lives on the GPU: the complete clouds are uploaded once and every step's (existing, missing, gt)
is cut from them there by ops.make_batch (csrc/batch_maker.hip) — the reference's slicing law and z-rotation, no loader
workers, no host-to-device copies and no host synchronisation per step.

    data = DeviceDataset("shapenet_2048.npz")                 # (M, 2048, 3) float32 [+ labels, names]
    for existing, missing, gt, labels in DeviceBatcher(data, 64, rotate=True):
        engine.step(existing, missing, gt, epoch)

The reference reads `.ply` files (datasets/shapenet.py) through a vendored reader; converting them to one array is a
one-time job of the user and not done here.
"""
import os

import numpy as np
import torch

from .. import ops
from .._lib import HipExtensionError


def _load(path):
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        return np.load(path), None, None
    if ext == ".npz":
        with np.load(path, allow_pickle=False) as z:
            if "clouds" not in z.files:
                raise ValueError(f"{path}: an .npz dataset holds 'clouds' (M,N,3) and optionally 'labels' (M), 'names'")
            return z["clouds"], (z["labels"] if "labels" in z.files else None), \
                ([str(n) for n in z["names"]] if "names" in z.files else None)
    raise ValueError(f"{path}: expected a .npy or .npz file")


class DeviceDataset:
    """M complete clouds of N points, resident on the device as one contiguous float32 (M,N,3) tensor.
    clouds: numpy array, CPU or CUDA tensor, or the path of a .npy (the array) / .npz ('clouds' [, 'labels', 'names']) file.
    labels: (M) integer category of each cloud; names: the categories' names (index = label)."""

    def __init__(self, clouds, labels=None, names=None, device=None):
        if isinstance(clouds, (str, os.PathLike)):
            clouds, file_labels, file_names = _load(os.fspath(clouds))
            labels = file_labels if labels is None else labels
            names = file_names if names is None else names
        t = torch.as_tensor(clouds)
        if t.dim() != 3 or t.size(2) != 3 or t.size(0) < 1 or t.size(1) < 2:
            raise ValueError(f"clouds must be (M,N,3) with M >= 1 and N >= 2, got {tuple(t.shape)}")
        if not (t.is_floating_point() or t.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)):
            raise ValueError(f"clouds must be numeric, got {t.dtype}")
        if device is None:
            device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.clouds = t.to(device=device, dtype=torch.float32).contiguous()
        if not bool(torch.isfinite(self.clouds).all()):          # once, at construction: the only check that reads the data
            raise ValueError("clouds contain non-finite values")
        self.labels = None
        if labels is not None:
            lab = torch.as_tensor(labels)
            if lab.dim() != 1 or lab.numel() != t.size(0) or lab.is_floating_point():
                raise ValueError("labels must be (M) integers, one per cloud")
            if int(lab.min()) < 0:
                raise ValueError("labels must be >= 0")
            self.labels = lab.to(device=self.clouds.device, dtype=torch.int64)
        self.names = None if names is None else [str(n) for n in names]
        if self.names is not None and self.labels is not None and int(self.labels.max()) >= len(self.names):
            raise ValueError("a label has no name")

    def __len__(self):
        return self.clouds.size(0)

    @property
    def n_points(self):
        return self.clouds.size(1)

    @property
    def device(self):
        return self.clouds.device

    def by_label(self):
        """{category name: DeviceDataset of that category's clouds} in label order — the per-category sets of val_epoch."""
        if self.labels is None:
            raise ValueError("by_label() needs labels")
        out = {}
        for k in torch.unique(self.labels).tolist():
            sel = self.labels == k
            name = self.names[k] if self.names is not None else str(k)
            out[name] = DeviceDataset(self.clouds[sel], self.labels[sel], self.names, device=self.device)
        return out


def epoch_plan(n_clouds, num_samples, batch_size, epoch, seed=0, rank=0, world=1, shuffle=True, drop_last=True, rotate=False,
               fresh_slices=False, device="cpu"):
    """This rank's items of one epoch, drawn once on `device`: (ids int32, streams int64, degrees int32 or None), each of
    this rank's length.  An epoch is every (cloud, scan), scan < num_samples, once over all ranks (the reference's
    len = clouds * num_samples); item = cloud * num_samples + scan.  The permutation and the degrees come from a
    torch.Generator seeded by (seed, epoch); rank r takes every world-th item from r.  drop_last cuts every rank to the
    same whole number of batches.  Stream id = item (the same split of a (cloud, scan) in every epoch, as the reference's
    pre-sliced files), or, with fresh_slices, epoch * clouds * num_samples + item."""
    if not (0 <= rank < world):
        raise ValueError(f"rank {rank} outside a world of {world}")
    total = n_clouds * num_samples
    gen = torch.Generator(device=device)
    gen.manual_seed((int(seed) * 1000003 + int(epoch)) % (2 ** 63))
    items = torch.randperm(total, generator=gen, device=device) if shuffle else torch.arange(total, device=device)
    degrees = torch.randint(0, 360, (total,), generator=gen, device=device, dtype=torch.int32) if rotate else None
    mine = items[rank::world]
    if degrees is not None:
        degrees = degrees[rank::world]
    if drop_last:
        keep = (total // world) // batch_size * batch_size
        mine = mine[:keep]
        degrees = None if degrees is None else degrees[:keep]
    ids = torch.div(mine, num_samples, rounding_mode="floor").to(torch.int32).contiguous()
    streams = (mine + int(epoch) * total if fresh_slices else mine).to(torch.int64).contiguous()
    return ids, streams, (None if degrees is None else degrees.contiguous())


class _EpochBatcher:
    """What DeviceBatcher and DeviceViewBatcher share: the epoch plan, the iteration and the prefetch machinery.  A subclass
    allocates self._sets (one output buffer set, two with prefetch) and states _make; _begin_epoch may add to the plan."""

    def __init__(self, dataset, batch_size, target, num_samples, rotate, shuffle, seed, rank, world, drop_last, fresh_slices,
                 prefetch, what):
        if not isinstance(dataset, DeviceDataset):
            raise TypeError("dataset must be a DeviceDataset")
        if not dataset.clouds.is_cuda:
            raise HipExtensionError(f"{type(self).__name__} needs a dataset on the GPU — {what} has no CPU path")
        if batch_size < 1 or num_samples < 1 or not (0 < target < dataset.n_points):
            raise ValueError("batch_size >= 1, num_samples >= 1 and 0 < target < N are required")
        if not (0 <= rank < world):
            raise ValueError(f"rank {rank} outside a world of {world}")
        self.dataset, self.batch_size, self.target, self.num_samples = dataset, int(batch_size), int(target), int(num_samples)
        self.rotate, self.shuffle, self.seed, self.rank, self.world = rotate, shuffle, int(seed), rank, world
        self.drop_last, self.fresh_slices, self.prefetch = drop_last, fresh_slices, prefetch
        self.epoch = 0
        dev = dataset.device
        self._rot = ops.rotation_table(dev) if rotate else None
        self._stream = self._ready = self._free = None
        if prefetch:
            # A further stream: at the runtime's four hardware queues it shares one with the streams already there (the
            # model's high-priority side stream keeps its own pool — see full_model._side_stream).
            self._stream = torch.cuda.Stream(device=dev)
            self._ready = [torch.cuda.Event() for _ in range(2)]
            self._free = [torch.cuda.Event() for _ in range(2)]

    def __len__(self):
        per_rank = len(range(self.rank, len(self.dataset) * self.num_samples, self.world))
        if self.drop_last:
            return (len(self.dataset) * self.num_samples // self.world) // self.batch_size
        return -(-per_rank // self.batch_size)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _begin_epoch(self, epoch, ids, streams):
        """What a subclass adds to the epoch's plan, per item of this rank (None: nothing)."""
        return None

    def _make(self, plan, k, bufs):
        """Batch k of the plan (ids, streams, degrees, labels, extra) into the buffer set bufs."""
        raise NotImplementedError

    def _cut(self, plan, k, bufs):
        """-> (lo, hi, out): the items of batch k and the buffer set cut to them (the last batch may be short)."""
        lo, hi = k * self.batch_size, min((k + 1) * self.batch_size, plan[0].numel())
        return lo, hi, (bufs if hi - lo == self.batch_size else {n: t[:hi - lo] for n, t in bufs.items()})

    def __iter__(self):
        data, dev = self.dataset, self.dataset.device
        epoch, self.epoch = self.epoch, self.epoch + 1
        ids, streams, degrees = epoch_plan(len(data), self.num_samples, self.batch_size, epoch, self.seed, self.rank, self.world,
                                           self.shuffle, self.drop_last, self.rotate, self.fresh_slices, dev)
        labels = None if data.labels is None else data.labels[ids.long()]
        plan = (ids, streams, degrees, labels, self._begin_epoch(epoch, ids, streams))
        n = -(-ids.numel() // self.batch_size)
        if not self.prefetch:
            for k in range(n):
                yield self._make(plan, k, self._sets[0])
            return
        cur, own = torch.cuda.current_stream(dev), self._stream

        def produce(k):
            with torch.cuda.stream(own):
                batch = self._make(plan, k, self._sets[k & 1])     # `own` runs the calls in order (one workspace is enough)
                self._ready[k & 1].record(own)
            return batch

        own.wait_stream(cur)                      # the epoch's plan, and whatever still reads the buffers
        nxt = produce(0) if n else None
        for k in range(n):
            batch = nxt
            cur = torch.cuda.current_stream(dev)
            cur.wait_event(self._ready[k & 1])
            if k + 1 < n:
                # the caller asked for batch k: its work on batch k-1 (same buffers as k+1) is all enqueued on `cur`
                self._free[(k + 1) & 1].record(cur)
                own.wait_event(self._free[(k + 1) & 1])
                nxt = produce(k + 1)
            yield batch
        torch.cuda.current_stream(dev).wait_stream(own)


class DeviceBatcher(_EpochBatcher):
    """Iterating yields one epoch of (existing (B,target,3), missing (B,N-target,3), gt (B,N,3), labels (B) or None) device
    tensors; every `iter()` is the next epoch (set_epoch() to choose).  Output buffers and the workspace are allocated once:
    a batch is valid until the next `next()`.  prefetch=True produces batch k+1 on the batcher's own stream into a second
    buffer set while the caller works on batch k (events order the two streams both ways); a batch is then still valid
    until the next `next()`.  failures() — the number of items for which no plane was accepted — is the only host
    synchronisation, on demand."""

    def __init__(self, dataset, batch_size, target=1024, num_samples=4, rotate=False, shuffle=True, seed=0, rank=0, world=1,
                 drop_last=True, fresh_slices=False, groups=None, max_candidates=400_000, prefetch=False):
        super().__init__(dataset, batch_size, target, num_samples, rotate, shuffle, seed, rank, world, drop_last, fresh_slices,
                         prefetch, "the batch maker")
        self.max_candidates = int(max_candidates)
        self.groups = ops.make_batch_default_groups(batch_size) if groups is None else int(groups)
        dev = dataset.device
        self._failed = torch.zeros((1,), dtype=torch.int32, device=dev)
        self._ws = ops.make_batch_workspace(self.batch_size, dataset.n_points, dev)
        self._sets = [ops.make_batch_buffers(self.batch_size, dataset.n_points, self.target, dev) for _ in range(2 if prefetch else 1)]

    def failures(self):
        """Items so far for which no plane was accepted below max_candidates (they were served as first-`target` / rest)."""
        return int(self._failed.item())

    def _make(self, plan, k, bufs):
        ids, streams, degrees, labels, _ = plan
        lo, hi, out = self._cut(plan, k, bufs)
        ex, mi, gt, _, _, _ = ops.make_batch(self.dataset.clouds, ids[lo:hi], streams[lo:hi], self.target,
                                             None if degrees is None else degrees[lo:hi], self._rot, self.seed,
                                             self.max_candidates, self.groups, out=out, ws=self._ws, failed=self._failed)
        return ex, mi, gt, (None if labels is None else labels[lo:hi])


class DeviceViewBatcher(_EpochBatcher):
    """DeviceBatcher's sibling whose `existing` part is the self-occluded view of a depth sensor (ops.make_view_batch,
    csrc/view_split.hip) where DeviceBatcher cuts with a random plane: the same (existing, missing, gt, labels) per batch, the
    same epochs, ranks, rotation and prefetch, so train_epoch and val_epoch take either.
    The frame of item (cloud, scan) is row `item` of ops.view_frames(clouds * num_samples, seed): the same view in every
    epoch; with fresh_slices the frames are drawn from (seed, epoch) instead.  They are uploaded once (once per epoch with
    fresh_slices).  The sensor sits at `distance` from the origin and its image of resolution^2 pixels is fitted to a sphere of
    `radius` about the origin (None: the dataset's largest point norm — one reduction and one host read, here); `window` as
    make_view_batch.  No item can fail: failures() is always 0."""

    def __init__(self, dataset, batch_size, target=1024, num_samples=4, rotate=False, shuffle=True, seed=0, rank=0, world=1,
                 drop_last=True, fresh_slices=False, distance=3.0, radius=None, resolution=32, window=1, prefetch=False):
        super().__init__(dataset, batch_size, target, num_samples, rotate, shuffle, seed, rank, world, drop_last, fresh_slices,
                         prefetch, "the viewpoint batch maker")
        if radius is None:
            radius = float(dataset.clouds.square().sum(-1).max().sqrt().item())
        self.distance, self.radius, self.resolution, self.window = float(distance), float(radius), int(resolution), int(window)
        self.half_extent = ops.view_half_extent(self.radius, self.distance)
        ops._check_view(self.distance, self.half_extent, resolution, window)
        dev = dataset.device
        self._frames = None                               # (epoch drawn for, (clouds * num_samples, 3, 3) on the device)
        self._sets = [ops.make_view_batch_buffers(self.batch_size, dataset.n_points, self.target, dev, side=False, occlusion=False)
                      for _ in range(2 if prefetch else 1)]

    def failures(self):
        return 0

    def frames(self, epoch):
        """The (clouds * num_samples, 3, 3) host frames of an epoch, row = item."""
        total = len(self.dataset) * self.num_samples
        return ops.view_frames(total, (self.seed, int(epoch)) if self.fresh_slices else self.seed)

    def _begin_epoch(self, epoch, ids, streams):
        drawn = epoch if self.fresh_slices else 0
        if self._frames is None or self._frames[0] != drawn:
            self._frames = (drawn, self.frames(epoch).to(self.dataset.device))
        total = len(self.dataset) * self.num_samples
        return self._frames[1][streams % total].contiguous()          # stream id = item (+ epoch * total): this rank's frames

    def _make(self, plan, k, bufs):
        ids, _, degrees, labels, frames = plan
        lo, hi, out = self._cut(plan, k, bufs)
        ex, mi, gt, _, _ = ops.make_view_batch(self.dataset.clouds, ids[lo:hi], frames[lo:hi], self.target,
                                               None if degrees is None else degrees[lo:hi], self._rot, self.distance,
                                               self.half_extent, self.resolution, self.window, out=out)
        return ex, mi, gt, (None if labels is None else labels[lo:hi])
