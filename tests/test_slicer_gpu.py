"""GPU: the on-device random-plane slicer (datasets/utils/dataset_generator.py:26-39).
The reference draws planes from numpy's global RNG, so parity is by properties: exact part sizes, a partition of the
input in original order, separation by the reported plane evaluated with the reference's formula, determinism per seed,
and the acceptance law (both orientations occur)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_slicer_partitions_exactly_and_in_order():
    from hyperpocket_amd.ops import slice_clouds
    g = torch.Generator(device="cuda").manual_seed(0)
    pts = torch.rand(48, 2048, 3, device="cuda", generator=g) - 0.5
    a, b, plane = slice_clouds(pts, 1024, seed=7)
    assert a.shape == (48, 1024, 3) and b.shape == (48, 1024, 3)
    P, A, Bn, pl = pts.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy(), plane.cpu().numpy()
    n_under_selected = 0
    for c in range(48):
        # reference formula: sign(dot(point, params) + bias) (HyperPlane.check_point)
        under = (P[c] @ pl[c, :3] + pl[c, 3]) > 0
        if under.sum() == 1024 and np.array_equal(P[c][under], A[c]):
            n_under_selected += 1
            assert np.array_equal(P[c][~under], Bn[c])
        else:
            assert (~under).sum() == 1024 and np.array_equal(P[c][~under], A[c]) and np.array_equal(P[c][under], Bn[c])
    assert 0 < n_under_selected <= 48
    a2, b2, _ = slice_clouds(pts, 1024, seed=7)
    assert torch.equal(a, a2) and torch.equal(b, b2)
    a3, _, _ = slice_clouds(pts, 1024, seed=8)
    assert not torch.equal(a, a3)


def test_slicer_uneven_target_and_dataset_generator_api():
    from hyperpocket_amd.datasets.utils.dataset_generator import SlicedDatasetGenerator
    g = torch.Generator(device="cuda").manual_seed(1)
    pts = torch.rand(333, 3, device="cuda", generator=g)
    part, rest = SlicedDatasetGenerator.generate_item(pts, 100, seed=3)
    assert part.shape == (100, 3) and rest.shape == (233, 3)
    allp = torch.cat([part, rest]).cpu().numpy()
    assert sorted(map(tuple, allp.tolist())) == sorted(map(tuple, pts.cpu().numpy().tolist()))
    batch = torch.rand(5, 2048, 3, device="cuda", generator=g) - 0.5
    ex, mi = SlicedDatasetGenerator.generate_batch(batch, 1024, seed=11)
    assert ex.shape == (5, 1024, 3) and mi.shape == (5, 1024, 3)


def test_slicer_with_the_reference_planes_is_the_reference_split_bit_for_bit():
    """N3, rule (f): tests/golden/slicer.npz holds what the reference's own SlicedDatasetGenerator.generate_item
    (datasets/utils/dataset_generator.py:29-39) returned under a seeded np.random, plus the candidate planes
    HyperPlane.get_random_plane drew for it.  hp_slice_clouds_planes classifies in float64 as check_point (:10-11):
    accepted-plane index and both parts must be IDENTICAL — through ops.slice_clouds and through the C ABI."""
    import ctypes
    from conftest import golden
    from hyperpocket_amd import load_library
    from hyperpocket_amd.datasets.utils.dataset_generator import SlicedDatasetGenerator
    from hyperpocket_amd.ops import slice_clouds
    from oracle.slicer_ref import slice_with_planes
    g = golden("slicer")
    lib = load_library()
    for name in g["cases"]:
        pts, planes = g[f"{name}_points"], g[f"{name}_planes"]
        want_a, want_b, want_idx = g[f"{name}_part_a"], g[f"{name}_part_b"], int(g[f"{name}_accepted"])
        target = want_a.shape[0]
        P = torch.from_numpy(pts).cuda()
        a, b, idx = slice_clouds(P.unsqueeze(0), target, planes=planes)
        assert int(idx[0]) == want_idx, (name, int(idx[0]), want_idx)
        assert np.array_equal(a[0].cpu().numpy(), want_a) and np.array_equal(b[0].cpu().numpy(), want_b), name
        # the reference-shaped call
        pa, pb = SlicedDatasetGenerator.generate_item(P, target, planes=planes)
        assert np.array_equal(pa.cpu().numpy(), want_a) and np.array_equal(pb.cpu().numpy(), want_b), name
        # raw C ABI, two clouds sharing the launch with DIFFERENT candidate lists: cloud 1 gets the list without its
        # first 3 candidates -> the accepted index shifts by 3, same parts
        if want_idx >= 3:
            R = planes.shape[0] - 3
            pl2 = torch.from_numpy(np.stack([planes[:R], planes[3:]])).cuda()
            P2 = P.unsqueeze(0).repeat(2, 1, 1).contiguous()
            N = pts.shape[0]
            A = torch.empty(2, target, 3, device="cuda"); Bt = torch.empty(2, N - target, 3, device="cuda")
            pi = torch.empty(2, dtype=torch.int32, device="cuda"); st = torch.empty(2, dtype=torch.int32, device="cuda")
            rc = lib.hp_slice_clouds_planes(2, N, target, ctypes.c_void_p(P2.data_ptr()), ctypes.c_void_p(pl2.data_ptr()), R,
                                            ctypes.c_void_p(A.data_ptr()), ctypes.c_void_p(Bt.data_ptr()),
                                            ctypes.c_void_p(pi.data_ptr()), ctypes.c_void_p(st.data_ptr()), None)
            assert rc == 0
            torch.cuda.synchronize()
            assert pi.tolist() == [want_idx, want_idx - 3] and st.tolist() == [0, 0], (name, pi.tolist())
            for c in range(2):
                assert np.array_equal(A[c].cpu().numpy(), want_a) and np.array_equal(Bt[c].cpu().numpy(), want_b), name
        # a candidate list that ends before the accepted plane: status 1 -> HipExtensionError, as documented
        from hyperpocket_amd import HipExtensionError
        if want_idx > 0:
            with pytest.raises(HipExtensionError):
                slice_clouds(P.unsqueeze(0), target, planes=planes[:want_idx])
    # seeded clouds beyond the fixture: the kernel against the numpy restatement of the reference (oracle/slicer_ref.py,
    # itself pinned by the fixture on CPU), planes drawn here the way the reference draws them
    rs = np.random.RandomState(5)
    for N, target in ((2048, 1024), (1000, 400), (64, 32), (4097, 2048)):
        B = 3
        pts = (rs.random_sample((B, N, 3)) - 0.5).astype(np.float32)
        R = 6000
        tri = rs.random_sample((B, R, 3, 3))
        cp = np.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0])
        planes = np.concatenate([cp, (cp * tri[:, :, 0]).sum(-1, keepdims=True)], -1)
        planes[:, :, 3] -= 0.5 * cp.sum(-1)                    # through the cloud's cube, so that a split exists within R
        want = [slice_with_planes(pts[c], planes[c], target) for c in range(B)]
        assert all(w[2] >= 0 for w in want), (N, target)      # seeded: every cloud finds its split within R
        a, b, idx = slice_clouds(torch.from_numpy(pts).cuda(), target, planes=planes)
        for c in range(B):
            assert int(idx[c]) == want[c][2], (N, target, c)
            assert np.array_equal(a[c].cpu().numpy(), want[c][0]) and np.array_equal(b[c].cpu().numpy(), want[c][1])


@pytest.mark.parametrize("N,target,draw", [(8192, 4096, 3), (257, 1, 5)])
def test_slicer_with_given_planes_at_the_cap_and_with_a_lone_last_candidate(N, target, draw):
    """The caller's-planes form at the documented cap N = 8192 (98 304 B of dynamic LDS) and at a one-point part, against
    oracle/slicer_ref.py, with R = 4k + 1 candidates: every cloud's list starts so that its accepted index is a multiple of
    four, and the list ends with the slowest cloud's accepted plane — the last round has that one candidate and three idle
    waves."""
    from hyperpocket_amd.ops import slice_clouds
    from oracle.slicer_ref import slice_with_planes
    rs = np.random.RandomState(N + target + 1000 * draw)      # (`draw`: the first seed at which all three clouds split within R0)
    B, R0 = 3, 8000
    pts = (rs.random_sample((B, N, 3)) - 0.5).astype(np.float32)
    tri = rs.random_sample((B, R0, 3, 3))
    cp = np.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0])
    planes = np.concatenate([cp, (cp * tri[:, :, 0]).sum(-1, keepdims=True)], -1)
    planes[:, :, 3] -= 0.5 * cp.sum(-1)                        # through the cloud's cube, so that a split exists within R0
    first = [slice_with_planes(pts[c], planes[c], target)[2] for c in range(B)]
    assert all(4 <= f < R0 - 4 for f in first), first          # seeded: every cloud finds its split
    start = [f % 4 for f in first]
    R = max(f - s for f, s in zip(first, start)) + 1
    assert R % 4 == 1 and all(s + R <= R0 for s in start)
    lists = np.stack([planes[c, s:s + R] for c, s in enumerate(start)])
    want = [slice_with_planes(pts[c], lists[c], target) for c in range(B)]
    assert [w[2] for w in want] == [f - s for f, s in zip(first, start)] and max(w[2] for w in want) == R - 1
    a, b, idx = slice_clouds(torch.from_numpy(pts).cuda(), target, planes=lists)
    assert idx.tolist() == [w[2] for w in want]
    for c in range(B):
        assert np.array_equal(a[c].cpu().numpy(), want[c][0]) and np.array_equal(b[c].cpu().numpy(), want[c][1]), c
    # one candidate fewer: the slowest cloud alone has none
    from hyperpocket_amd import HipExtensionError
    with pytest.raises(HipExtensionError, match="1 cloud"):
        slice_clouds(torch.from_numpy(pts).cuda(), target, planes=lists[:, :R - 1])
