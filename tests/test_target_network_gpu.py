"""The decoder kernels (csrc/target_fused.hip: hp_target_fused_forward / hp_target_fused_backward; the layered path
hp_target_forward / hp_target_backward of csrc/model.hip) against an fp64 evaluation of the same decoder, per cloud and
per parameter block, at every launch geometry the fused backward's launcher can choose.

Yardstick: oracle/hyperpocket_ref.py target_forward per cloud on theta.double(), pts.double() on the CPU, autograd of
(y * grad_y.double()).sum(), the gradient cut into the ten blocks W1 b1 ... W5 b5 of target_layout().  A gradient
comparison is  max|got - want| <= BAR * max|want|  over one block of one cloud; a block whose fp64 gradient is identically
zero must come back exactly zero.  BAR = 2e-5 is the bar the older decoder tests apply to the whole 19 011-vector
(grad_close(tol=2e-5)); it is not derived from the kernels.  Forward comparisons keep the bars of
test_target_fused_forward_f16_pipe_is_as_close_to_fp64_as_the_fp32_kernel, per cloud.

Inputs are made well-posed first (well_posed): a point with a hidden unit whose fp64 pre-activation lies within
1e-4 * rms of zero is re-drawn, because an fp32 evaluation may take the other side of that ReLU and move the point's whole
contribution (1e-3 of a block at 64 clouds); nothing is dropped or masked out of a comparison.

Measured on an MI355X (every test prints its figures; `-s` shows them).  The bars are not tightened to these.
  worst per-cloud per-block gradient ratio over all 48 tests (bar 2e-5):
      fused vs fp64 2.9e-6, layered vs fp64 3.0e-6, fused vs layered 3.0e-6 — all three at theta * 0.01, points * 1e-3,
      grad_y * 1e4, block W2; over the launch geometries alone 2.5e-6 / 2.5e-6 / 2.7e-6 (100 x 700 and 32 x 8192, W4);
      trained operating point 6.2e-7 / 5.1e-7 / 7.0e-7; one point per cloud 4.2e-7 / 4.2e-7 / 0 (bit-identical).
  worst per-cloud forward error (bar 3e-6): f16 pipe 1.1e-6, fp32 kernel 1.0e-6, layered 1.2e-6.
  fragile on the first pass: 2.2-3.1 % at unit scales (N >= 127), 2.8-3.0 % at theta * 1.5, points * 30, 0.1-0.6 % at
      theta * 0.01, points * 1e-3 (after 1-3 theta re-draws, see redraw_undecided_theta), 2.05 % on the trained fixture's own
      points and 2.6 % on fresh unit-sphere points under the trained theta; 0-5 re-draw passes.
  smallest block relative to the vector's max|grad| (what a whole-vector bar would let slip): theta * 0.05: W1 b1 W2 1e-3;
      theta * 1.5, points * 30: b4 3e-5, b5 2.4e-6; theta * 0.01, points * 1e-3: W1 1e-9, W2 7e-7, b1 2e-6.
  trained operating point (tests/golden/model_trained.npz): max|theta| per block W1 0.41, b1 0.35, W2 0.34, b2 0.22, W3 0.30,
      b3 0.18, W4 0.27, b4 0.20, W5 0.45, b5 0.55; block max|grad| / vector max|grad| under the Chamfer gradient, min..max over
      clouds: W1 0.18..0.74, b1 0.33..0.90, W2 0.15..0.40, b2 0.30..1.0, W3 0.11..0.25, b3 0.29..0.69, W4 0.15..0.42,
      b4 0.33..0.70, W5 0.51..1.0, b5 0.93..1.0 — the blocks lie within 10x of each other there, as at theta ~ 0.2 * randn.
  wall time of the module: 12 s (CPU references included).
"""
import ctypes
import math
import time
import zlib

import pytest
import torch

from conftest import fixture_state_, golden

pytestmark = pytest.mark.gpu

T = 19011
LD = T + 13                      # padded theta rows, as a caller slicing a wider buffer hands them over
TAIL = 4096                      # sentinel floats behind every output buffer
SENT = 7.0
BAR = 2e-5
MARGIN = 1e-4
BLOCK_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "W5", "b5")
CH = (ctypes.c_int * 4)(32, 64, 128, 64)


# ----------------------------------------------------------------------------------------------- plumbing
def _lib():
    from hyperpocket_amd._lib import load_library
    lib = load_library()
    for name in ("hp_target_fused_workspace_floats", "hp_target_saved_floats", "hp_target_backward_workspace_floats"):
        getattr(lib, name).restype = ctypes.c_long
    return lib


def block_slices(ref):
    layout, total = ref.target_layout()
    assert total == T
    out = []
    for wo, o, k, bo in layout:
        out += [(wo, wo + o * k), (bo, bo + o)]
    return out


def uniform_cube(pscale):
    return lambda n, gen: (torch.rand(n, 3, generator=gen) * 2 - 1) * pscale


def unit_sphere(n, gen):
    """The decoder input of an epoch past the progressive normalisation (utils/points.py): uniform in the unit ball by
    rejection from the cube, every point then pushed out onto the sphere."""
    out = torch.empty(0, 3)
    while out.size(0) < n:
        p = torch.rand(3 * n + 8, 3, generator=gen) * 2 - 1
        r = p.norm(dim=1)
        keep = (r < 1) & (r > 1e-3)
        out = torch.cat([out, p[keep] / r[keep, None]])
    return out[:n].contiguous()


def preacts64(ref, theta, pts):
    """fp64 pre-activations of the four hidden layers, batched over clouds: [(B, N, C_l)]."""
    layout, _ = ref.target_layout()
    B = theta.size(0)
    h, zs = pts.double(), []
    for wo, o, k, bo in layout[:4]:
        W = theta[:, wo:wo + o * k].double().view(B, o, k)
        b = theta[:, bo:bo + o].double().view(B, 1, o)
        z = torch.baddbmm(b, h, W.transpose(1, 2))
        zs.append(z)
        h = torch.relu(z)
    return zs


def fragile_points(ref, theta, pts, exempt=None):
    """(B, N) bool: a point is fragile if any hidden unit has |z| <= MARGIN * rms(z over that layer of that cloud).
    exempt (B, 4) bool: layers put at exactly zero on purpose."""
    frag = torch.zeros(pts.shape[:2], dtype=torch.bool)
    for l, z in enumerate(preacts64(ref, theta, pts)):
        rms = z.pow(2).mean(dim=(1, 2)).sqrt()
        f = (z.abs() <= MARGIN * rms[:, None, None]).any(dim=2)
        if exempt is not None:
            f &= ~exempt[:, l, None]
        frag |= f
    return frag


def well_posed(ref, theta, pts, draw, gen, label, exempt=None, cap=0.05):
    """Re-draws the fragile points of `pts` in place from the case's own distribution.  Asserts the three conditions that
    keep it from quietly eating a case: at most `cap` of the points fragile on the first pass, at most 8 passes, none
    left.  Returns (first-pass share, passes)."""
    total = pts.size(0) * pts.size(1)
    first, passes = None, 0
    while True:
        frag = fragile_points(ref, theta, pts, exempt)
        n = int(frag.sum())
        if first is None:
            first = n / total
            assert first <= cap, f"{label}: {first:.2%} of the points fragile on the first pass (cap {cap:.0%})"
        if n == 0:
            break
        assert passes < 8, f"{label}: {n} fragile points left after 8 passes"
        pts[frag] = draw(n, gen)
        passes += 1
    assert not fragile_points(ref, theta, pts, exempt).any()
    print(f"[margin] {label}: {first:.2%} fragile on the first pass, {passes} re-draw passes")
    return first, passes


def redraw_undecided_theta(ref, theta, pts, tscale, gen, label, share=0.25):
    """Where the biases dominate the pre-activations (theta * 0.01 on points * 1e-3: z = b + O(1e-5)) a unit with b next to
    zero is fragile at most points of its cloud whichever points are drawn, so re-drawing points cannot help: such a
    cloud's theta is re-drawn instead, as for the exact cases, at most 8 times.  A cloud counts as such when more than
    `share` of its own points are fragile — ten times what the random cases show (2-3 %), and the share above which 8
    point re-draws would not empty a cloud of these sizes (8192 * 0.25**8 < 1).  The points keep well_posed's conditions."""
    for attempt in range(9):
        bad = fragile_points(ref, theta, pts).float().mean(dim=1) > share
        if not bad.any():
            if attempt:
                print(f"[margin] {label}: theta of some clouds re-drawn, {attempt} rounds")
            return
        assert attempt < 8, f"{label}: clouds {bad.nonzero().flatten().tolist()} still have undecided units after 8 theta draws"
        theta[bad] = torch.randn(int(bad.sum()), T, generator=gen) * tscale


def reference64(ref, theta, pts, gy):
    """(y, grad_theta) in fp64 on the CPU: the oracle's decoder per cloud, autograd."""
    th = theta.double().requires_grad_(True)
    p = pts.double()
    y = torch.stack([ref.target_forward(th[j], p[j]) for j in range(theta.size(0))])
    (y * gy.double()).sum().backward()
    return y.detach(), th.grad


_CASES = {}


def make_case(ref, B, N, tscale=0.2, pscale=1.0, gscale=1.0):
    """Dense case: theta ~ tscale * randn, points uniform in [-1, 1]^3 * pscale, grad_y ~ gscale * randn; seeded by its
    own parameters, made well-posed, fp64 reference computed once and shared by every test that uses the shape."""
    key = (B, N, tscale, pscale, gscale)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
        theta = torch.randn(B, T, generator=gen) * tscale
        draw = uniform_cube(pscale)
        pts = draw(B * N, gen).view(B, N, 3).contiguous()
        gy = torch.randn(B, N, 3, generator=gen) * gscale
        redraw_undecided_theta(ref, theta, pts, tscale, gen, f"B={B} N={N} theta*{tscale} pts*{pscale}")
        first, passes = well_posed(ref, theta, pts, draw, gen, f"B={B} N={N} theta*{tscale} pts*{pscale}")
        y64, g64 = reference64(ref, theta, pts, gy)
        _CASES[key] = dict(B=B, N=N, theta=theta, pts=pts, gy=gy, y64=y64, g64=g64, first=first, passes=passes)
    return _CASES[key]


def padded(theta):
    wide = torch.full((theta.size(0), LD), float("nan"))
    wide[:, :T] = theta
    return wide.cuda()


def fused_geometry(lib, B, N):
    """(blocks, S, iters) of the fused backward, S read back from the library's workspace query."""
    ws = lib.hp_target_fused_workspace_floats(B, N)
    assert ws % (B * T) == 0
    S = ws // (B * T)
    blocks = (N + 127) // 128
    return blocks, S, (blocks + S - 1) // S


def fused_forward(lib, f16, theta_d, theta_ld, pts_d):
    """y (B, N, 3) on the CPU.  y is pre-filled with NaN (every row < N must be written) and carries a sentinel tail."""
    from hyperpocket_amd._lib import call, current_stream
    B, N = pts_d.shape[:2]
    buf = torch.full((B * N * 3 + TAIL,), float("nan"), device="cuda")
    buf[B * N * 3:] = SENT
    prev = lib.hp_target_fused_set_f16(f16)
    try:
        call("hp_target_fused_forward", B, N, theta_d, theta_ld, pts_d, buf, current_stream(buf.device))
        torch.cuda.synchronize()
    finally:
        lib.hp_target_fused_set_f16(prev)
    assert torch.all(buf[B * N * 3:] == SENT), "fused forward wrote behind y"
    y = buf[:B * N * 3].view(B, N, 3)
    assert torch.isfinite(y).all(), "fused forward left rows of y unwritten (or not finite)"
    return y.cpu()


def fused_backward(lib, theta_d, theta_ld, pts_d, gy_d, calls=2):
    """grad_theta (B, T) on the GPU.  Workspace NaN-filled before every call (each partial must be written by its own
    workgroup, empty ones included) with a sentinel tail; grad_theta's row padding keeps its sentinel; `calls` calls are
    bit-identical."""
    from hyperpocket_amd._lib import call, current_stream
    B, N = pts_d.shape[:2]
    nws = lib.hp_target_fused_workspace_floats(B, N)
    outs = []
    for _ in range(calls):
        ws = torch.full((nws + TAIL,), float("nan"), device="cuda")
        ws[nws:] = SENT
        gth = torch.full((B, theta_ld), SENT, device="cuda")
        call("hp_target_fused_backward", B, N, theta_d, theta_ld, pts_d, gy_d, gth, ws, current_stream(ws.device))
        torch.cuda.synchronize()
        assert torch.all(ws[nws:] == SENT), "fused backward wrote behind its workspace"
        assert not torch.isnan(ws[:nws]).any(), "a workgroup did not write its whole partial"
        assert torch.all(gth[:, T:] == SENT), "fused backward wrote into grad_theta's row padding"
        outs.append(gth[:, :T])
    for o in outs[1:]:
        assert torch.equal(outs[0], o), "fused backward is not bit-identical run to run"
    return outs[0]


def layered(lib, theta_d, theta_ld, pts_d, gy_d, calls=2):
    """(y, grad_theta (B, T)) of hp_target_forward / hp_target_backward, same buffer discipline as the fused calls."""
    from hyperpocket_amd._lib import call, current_stream
    B, N = pts_d.shape[:2]
    st = current_stream(pts_d.device)
    nact = lib.hp_target_saved_floats(B, N, 4, CH)
    nws = lib.hp_target_backward_workspace_floats(B, N, 4, CH)
    assert nact == B * N * 288 and nws > 0
    acts = torch.full((nact + TAIL,), float("nan"), device="cuda")
    acts[nact:] = SENT
    ybuf = torch.full((B * N * 3 + TAIL,), float("nan"), device="cuda")
    ybuf[B * N * 3:] = SENT
    call("hp_target_forward", B, N, 4, CH, theta_d, theta_ld, pts_d, acts, ybuf, st)
    torch.cuda.synchronize()
    assert torch.all(acts[nact:] == SENT) and torch.all(ybuf[B * N * 3:] == SENT), "layered forward wrote out of bounds"
    y = ybuf[:B * N * 3].view(B, N, 3)
    assert torch.isfinite(y).all() and torch.isfinite(acts[:nact]).all()
    outs = []
    for _ in range(calls):
        ws = torch.full((nws + TAIL,), float("nan"), device="cuda")
        ws[nws:] = SENT
        gth = torch.full((B, theta_ld), SENT, device="cuda")
        call("hp_target_backward", B, N, 4, CH, theta_d, theta_ld, pts_d, acts, gy_d, gth, ws, st)
        torch.cuda.synchronize()
        assert torch.all(ws[nws:] == SENT), "layered backward wrote behind its workspace"
        assert torch.all(gth[:, T:] == SENT), "layered backward wrote into grad_theta's row padding"
        outs.append(gth[:, :T])
        del ws
    for o in outs[1:]:
        assert torch.equal(outs[0], o), "layered backward is not bit-identical run to run"
    return y.cpu(), outs[0]


def block_ratios(ref, got, want, scale_of=None):
    """(B, 10) of max|got - want| / max|scale_of| per cloud and block (scale_of: the fp64 gradient; default `want`).
    A block whose fp64 gradient is identically zero must be exactly zero in `got`: reported as 0, or inf if it is not."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    scale_of = want if scale_of is None else scale_of.double()
    out = torch.zeros(got.size(0), 10, dtype=torch.float64)
    for i, (a, b) in enumerate(block_slices(ref)):
        scale = scale_of[:, a:b].abs().amax(dim=1)
        err = (got[:, a:b] - want[:, a:b]).abs().amax(dim=1)
        err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
        zero = scale == 0
        exact = (got[:, a:b] == 0).all(dim=1)
        out[:, i] = torch.where(zero, torch.where(exact, torch.zeros_like(err), torch.full_like(err, float("inf"))),
                                err / scale.clamp_min(1e-300))
    return out


def assert_blocks(ref, got, want, label, scale_of=None, bar=BAR):
    r = block_ratios(ref, got, want, scale_of)
    worst = r.max().item()
    j, i = divmod(int(r.argmax()), 10)
    print(f"[grad] {label}: worst per-cloud per-block ratio {worst:.2e} (cloud {j}, block {BLOCK_NAMES[i]})")
    bad = (r > bar).nonzero().tolist()
    assert not bad, (f"{label}: {len(bad)} (cloud, block) pairs above {bar:.0e}; worst {worst:.2e} at cloud {j}, block "
                     f"{BLOCK_NAMES[i]}; first few: " + ", ".join(f"({c}, {BLOCK_NAMES[k]}) {r[c, k]:.2e}" for c, k in bad[:6]))
    return worst


def cloud_errors(y, y64):
    """(B,) max|y - y64| / max|y64| per cloud."""
    y64 = y64.double()
    scale = y64.abs().amax(dim=(1, 2)).clamp_min(1e-300)
    return (y.double() - y64).abs().amax(dim=(1, 2)) / scale


def assert_forward(case, lib, label, theta_d=None):
    """Both fused forward kernels against fp64 at the forward bars, per cloud."""
    theta_d = padded(case["theta"]) if theta_d is None else theta_d
    pts_d = case["pts"].cuda()
    err = {f16: cloud_errors(fused_forward(lib, f16, theta_d, LD, pts_d), case["y64"]) for f16 in (1, 0)}
    print(f"[fwd] {label}: worst per-cloud error, f16 pipe {err[1].max():.2e}, fp32 kernel {err[0].max():.2e}")
    assert (err[1] <= 3e-6).all(), f"{label}: f16-pipe forward {err[1].max():.2e} of a cloud's max|y|"
    assert (err[1] <= 3 * err[0] + 2e-7).all(), f"{label}: f16 pipe {err[1].tolist()} against fp32 kernel {err[0].tolist()}"
    assert (err[0] <= 3e-6).all(), f"{label}: fp32 forward {err[0].max():.2e} of a cloud's max|y|"
    return err


def assert_backward_all(ref, lib, case, label):
    """Fused and layered backward against fp64 and against each other, per cloud and block; returns the three worst ratios."""
    theta_d, pts_d, gy_d = padded(case["theta"]), case["pts"].cuda(), case["gy"].cuda()
    gf = fused_backward(lib, theta_d, LD, pts_d, gy_d)
    yl, gl = layered(lib, theta_d, LD, pts_d, gy_d)
    el = cloud_errors(yl, case["y64"])
    print(f"[fwd] {label}: layered forward, worst per-cloud error {el.max():.2e}")
    assert (el <= 1e-5).all(), f"{label}: layered forward {el.max():.2e} of a cloud's max|y|"
    wf = assert_blocks(ref, gf, case["g64"], label + " fused vs fp64")
    wl = assert_blocks(ref, gl, case["g64"], label + " layered vs fp64")
    wx = assert_blocks(ref, gf, gl, label + " fused vs layered", scale_of=case["g64"])
    return wf, wl, wx


# ----------------------------------------------------------------------------------------------- 1, 2: launch geometries
# (B, N, the classes of the fused backward's launch the case is there for)
GEOMETRIES = [
    (1, 1, {"one-iteration", "ragged-tail"}),
    (1, 127, {"one-iteration", "ragged-tail"}),
    (1, 128, {"one-iteration", "full-tail"}),
    (1, 129, {"one-iteration", "ragged-tail"}),
    (3, 333, {"one-iteration", "ragged-tail"}),
    (64, 2048, {"multi-iteration", "full-tail", "no-empty-workgroup"}),          # the metric's shape
    (32, 2048, {"multi-iteration", "full-tail", "no-empty-workgroup"}),          # BASELINE configs[1]
    (100, 700, {"multi-iteration", "ragged-tail", "no-empty-workgroup"}),        # ragged last iteration
    (40, 1300, {"multi-iteration", "mid-loop-break", "empty-workgroups"}),
    (17, 2049, {"multi-iteration", "mid-loop-break", "empty-workgroups", "one-point-block"}),
    (2, 4100, {"multi-iteration", "empty-workgroups"}),                          # N > 2048 at small B
    (257, 300, {"multi-iteration", "one-workgroup-per-cloud", "ragged-tail"}),   # B above the CU count
    (32, 8192, {"multi-iteration", "full-tail", "no-empty-workgroup"}),          # the stress workload's N
]


def geometry_classes(blocks, S, iters, B, N):
    c = set()
    if iters == 1 and S == blocks:
        c.add("one-iteration")
    if iters > 1:
        c.add("multi-iteration")
    c.add("ragged-tail" if N % 128 else "full-tail")
    if N % 128 == 1:
        c.add("one-point-block")
    owners = (blocks + iters - 1) // iters          # workgroups that own at least one block
    if iters > 1 and blocks % iters:
        c.add("mid-loop-break")                     # workgroup blocks // iters leaves its loop at `if (p0 >= N) break`
    c.add("empty-workgroups" if owners < S else "no-empty-workgroup")
    if S == 1 and B > 256:
        c.add("one-workgroup-per-cloud")
    return c


@pytest.mark.parametrize("B,N,classes", GEOMETRIES, ids=[f"{b}x{n}" for b, n, _ in GEOMETRIES])
def test_backward_launch_geometries_vs_fp64(ref, B, N, classes):
    """Test 1: every launch class of the fused backward (single iteration with tails; carried accumulators; ragged last
    iteration; mid-loop break; workgroups that own no point and must still write a zero partial; one workgroup per cloud),
    fused and layered against fp64 per cloud and block, and against each other."""
    lib = _lib()
    blocks, S, iters = fused_geometry(lib, B, N)
    have = geometry_classes(blocks, S, iters, B, N)
    print(f"[geometry] B={B} N={N}: blocks={blocks} S={S} iters={iters} empty={S - (blocks + iters - 1) // iters} {sorted(have)}")
    assert classes <= have, (f"B={B}, N={N} launches as S={S}, iters={iters} over {blocks} blocks and no longer is "
                             f"{sorted(classes - have)}: choose a shape that still covers that class")
    assert_backward_all(ref, lib, make_case(ref, B, N), f"B={B} N={N}")


@pytest.mark.parametrize("B,N", [(b, n) for b, n, _ in GEOMETRIES], ids=[f"{b}x{n}" for b, n, _ in GEOMETRIES])
def test_forward_launch_geometries_vs_fp64(ref, B, N):
    """Test 2: the f16-pipe and fp32 forward kernels at the same shapes (100 x 700: two iterations per workgroup with a ragged
    second workgroup; 257 x 300: more iterations per workgroup than there are 256-point blocks), per cloud against fp64."""
    lib = _lib()
    blocks = (N + 255) // 256
    per = max(1, (blocks * B + 255) // 256)         # the launcher's arithmetic, stated here only to print the geometry
    print(f"[geometry] forward B={B} N={N}: 256-point blocks={blocks}, iterations per workgroup={per}")
    assert_forward(make_case(ref, B, N), lib, f"B={B} N={N}")


# ----------------------------------------------------------------------------------------------- 3: scales
@pytest.mark.parametrize("gscale", [1e-6, 1.0, 1e4])
@pytest.mark.parametrize("tscale,pscale", [(0.2, 1.0), (0.05, 1.0), (1.5, 30.0), (0.01, 1e-3)])
def test_backward_scales_vs_fp64(ref, tscale, pscale, gscale):
    """Test 3: the forward test's four (theta scale, point scale) pairs crossed with upstream gradient scales, where the ten
    blocks differ by up to 1e5 in magnitude and a whole-vector bar lets the small ones be wrong by their own size."""
    B, N = 40, 1300
    case = make_case(ref, B, N, tscale, pscale, gscale)
    rel = torch.stack([case["g64"][:, a:b].abs().amax(dim=1) for a, b in block_slices(ref)], 1)
    rel = (rel / rel.amax(dim=1, keepdim=True)).amin(dim=0)
    print("[scale] smallest block max|grad| / vector max|grad| over clouds: " +
          " ".join(f"{n}={v:.1e}" for n, v in zip(BLOCK_NAMES, rel.tolist())))
    assert_backward_all(ref, _lib(), case, f"theta*{tscale} pts*{pscale} grad_y*{gscale}")


# ----------------------------------------------------------------------------------------------- 4: trained operating point
def _trained_theta():
    """theta (4, T) as the product computes it for the clouds of tests/golden/model_trained.npz: encoders and hypernetwork
    on the GPU at the fixture's state; from here on theta is an input to both sides."""
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel
    g = golden("model_trained")
    enc = lambda size: {"output_size": size, "use_bias": True, "relu_slope": 0.2}
    torch.manual_seed(int(g["seed"]))
    model = FullModel({"random_encoder": enc(int(g["random_out"])), "real_encoder": enc(int(g["real_out"])),
                       "hyper_network": {"use_bias": True, "relu_slope": 0.2},
                       "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                                          "layer_out_channels": [32, 64, 128, 64]},
                       "target_network_input": {"constant": False,
                                                "normalization": {"enable": True, "type": "progressive", "epoch": 100}}})
    model.apply(weights_init)
    model = model.cuda()
    fixture_state_(model.state_dict(), g)
    model.train()
    seen = []
    hook = model.hyper_network.register_forward_hook(lambda m, i, o: seen.append(o.detach()))
    try:
        gt = torch.from_numpy(g["gt"]).cuda()
        model(torch.from_numpy(g["existing"]).cuda(), torch.from_numpy(g["missing"]).cuda(), list(gt.shape), int(g["epoch"]),
              torch.device("cuda"), points=torch.from_numpy(g["points"]).cuda(), eps=torch.from_numpy(g["eps"]).cuda())
    finally:
        hook.remove()
    theta = seen[0].cpu()
    assert theta.shape == (4, T)
    want = torch.from_numpy(g["theta"])
    assert (theta - want).abs().max().item() <= 1e-4 * want.abs().max().item()      # the fixture's own theta, loosely
    return theta, g


def _chamfer_grad(ref, gt, y64):
    """d(0.05 * Chamfer(gt, y)) / dy at the fp64 y: the upstream gradient of the training step (core/epoch_loops.py), fp32."""
    y = y64.clone().requires_grad_(True)
    (0.05 * ref.chamfer_loss(y, gt.double())).backward()
    return y.grad.float()


def _report_blocks(ref, g64, label):
    rel = torch.stack([g64[:, a:b].abs().amax(dim=1) for a, b in block_slices(ref)], 1)
    rel = rel / rel.amax(dim=1, keepdim=True)
    print(f"[trained] {label}: block max|grad| / vector max|grad|, min..max over clouds: " +
          " ".join(f"{n}={lo:.1e}..{hi:.1e}" for n, lo, hi in zip(BLOCK_NAMES, rel.amin(0).tolist(), rel.amax(0).tolist())))


def test_trained_operating_point_vs_fp64(ref):
    """Test 4: theta at its trained scale.  grad_y is the Chamfer gradient of the step, computed by the oracle in fp64 from
    the fp64 y.  (a) the fixture's 4 clouds with its own 256 decoder points (single iteration); (b) the 4 theta rows repeated
    to B = 40 with 1300 freshly drawn points per cloud on the unit sphere (the fixture's epoch is past the progressive
    normalisation), a multi-iteration launch with a mid-loop break and an empty workgroup."""
    lib = _lib()
    theta4, g = _trained_theta()
    gen = torch.Generator().manual_seed(4242)
    print("[trained] theta blocks max|theta|: " + " ".join(
        f"{n}={theta4[:, a:b].abs().max():.2e}" for n, (a, b) in zip(BLOCK_NAMES, block_slices(ref))))
    cases = []
    # (a): the margin helper's 5 % cap was measured on random theta only; if the trained theta breaks it on the fixture's points
    # the share is reported and the case rests on the freshly drawn points alone — the cap stays
    pts = torch.from_numpy(g["points"]).clone()
    share = fragile_points(ref, theta4, pts).float().mean().item()
    print(f"[trained] fixture points: {share:.2%} fragile on the first pass")
    if share <= 0.05:
        well_posed(ref, theta4, pts, unit_sphere, gen, "trained, fixture points")
        cases.append(("fixture 4x256", theta4, pts, torch.from_numpy(g["gt"])))
    else:
        print("[trained] fixture points exceed the 5 % cap: the fixture-point case is not compared")
    # (b)
    B, N = 40, 1300
    blocks, S, iters = fused_geometry(lib, B, N)
    assert iters > 1, "choose a shape that still launches more than one iteration per workgroup"
    theta = theta4.repeat(10, 1)
    pts = unit_sphere(B * N, gen).view(B, N, 3).contiguous()
    well_posed(ref, theta, pts, unit_sphere, gen, "trained, 40 x 1300 on the unit sphere")
    cases.append(("repeated 40x1300", theta, pts, torch.from_numpy(g["gt"]).repeat(10, 1, 1)))
    for label, theta, pts, gt in cases:
        y64, _ = reference64(ref, theta, pts, torch.zeros_like(pts))
        gy = _chamfer_grad(ref, gt, y64)
        y64, g64 = reference64(ref, theta, pts, gy)
        _report_blocks(ref, g64, label)
        case = dict(theta=theta, pts=pts, gy=gy, y64=y64, g64=g64)
        assert_forward(case, lib, "trained " + label)
        assert_backward_all(ref, lib, case, "trained " + label)


# ----------------------------------------------------------------------------------------------- 5: where each point lands
ONE_HOT_POINTS = [0, 1, 31, 32, 63, 64, 95, 96, 127, 128, 129, 255, 256, 1279, 1280, 1299,          # stage rows, halves, waves, tails
                  389, 454, 511, 673, 704, 897, 993, 1183, 1252,                                   # second iteration of workgroups 1..4
                  296, 575, 833, 1151, 200, 300, 450, 600, 750, 900, 1000, 1100, 1200, 1290, 160]


def test_backward_one_hot_points_vs_fp64(ref):
    """Test 5: 40 clouds share one theta and one point set; cloud j's grad_y is zero except one component of point p_j.  Each
    cloud's gradient is one point's analytic gradient — no summation — so a point staged into the wrong row, half or wave is
    an O(1) error in that cloud."""
    lib = _lib()
    B, N = 40, 1300
    assert len(ONE_HOT_POINTS) == B and max(ONE_HOT_POINTS) < N
    blocks, S, iters = fused_geometry(lib, B, N)
    later = sorted({(p // 128) // iters for p in ONE_HOT_POINTS if (p // 128) % iters})
    print(f"[geometry] one-hot: S={S} iters={iters}; workgroups probed beyond their first iteration: {later}")
    assert iters > 1 and len(later) >= 3, "choose points that still land in later iterations of several workgroups"
    gen = torch.Generator().manual_seed(55)
    theta1 = torch.randn(1, T, generator=gen) * 0.2
    draw = uniform_cube(1.0)
    pts1 = draw(N, gen).view(1, N, 3).contiguous()
    well_posed(ref, theta1, pts1, draw, gen, "one-hot point set")
    theta, pts = theta1.repeat(B, 1), pts1.repeat(B, 1, 1)
    gy = torch.zeros(B, N, 3)
    for j, p in enumerate(ONE_HOT_POINTS):
        gy[j, p, j % 3] = (-1.0) ** j * (0.5 + j / B)
    y64, g64 = reference64(ref, theta, pts, gy)
    assert (g64.abs().amax(dim=1) > 0).all()
    assert_backward_all(ref, lib, dict(theta=theta, pts=pts, gy=gy, y64=y64, g64=g64), "one-hot")


# ----------------------------------------------------------------------------------------------- 6: exact cases
def _special_theta(ref, gen, kind, l):
    """theta of one cloud with layer l (1-based) dead (`kind` = "dead": b_l = -1e3) or at exactly zero ("zero": W_l = 0, b_l = 0).
    Every layer above then sees the same input at every point, so whether its units are fragile depends on theta alone:
    theta is re-drawn (at most 8 attempts) until those layers hold the margin."""
    layout, _ = ref.target_layout()
    wo, o, k, bo = layout[l - 1]
    probe = torch.zeros(1, 1, 3)
    for _ in range(8):
        th = torch.randn(1, T, generator=gen) * 0.2
        if kind == "dead":
            th[0, bo:bo + o] = -1e3
        else:
            th[0, wo:wo + o * k] = 0.0
            th[0, bo:bo + o] = 0.0
        zs = preacts64(ref, th, probe)
        above = [z for i, z in enumerate(zs) if i + 1 > l]
        if all(bool((z.abs() > MARGIN * z.pow(2).mean().sqrt()).all()) for z in above):
            return th[0]
    raise AssertionError(f"no theta with layer {l} {kind} holds the margin above it in 8 attempts")


def _exact_case(ref):
    if "exact" in _CASES:
        return _CASES["exact"]
    B, N = 40, 1300
    gen = torch.Generator().manual_seed(606)
    theta = torch.randn(B, T, generator=gen) * 0.2
    exempt = torch.zeros(B, 4, dtype=torch.bool)
    spec = {0: ("dead", 4), 1: ("dead", 2), 2: ("zero", 1), 3: ("zero", 2), 4: ("zero", 3), 5: ("zero", 4)}
    for j, (kind, l) in spec.items():
        theta[j] = _special_theta(ref, gen, kind, l)
        exempt[j, l - 1] = kind == "zero"
    draw = uniform_cube(1.0)
    pts = draw(B * N, gen).view(B, N, 3).contiguous()
    gy = torch.randn(B, N, 3, generator=gen)
    well_posed(ref, theta, pts, draw, gen, "exact cases", exempt=exempt)
    zs = preacts64(ref, theta, pts)
    assert (zs[3][0] < 0).all() and (zs[1][1] < 0).all()                 # the dead layers are dead at every point
    for j, (kind, l) in spec.items():
        if kind == "zero":
            assert (zs[l - 1][j] == 0).all()                             # exactly zero, in any arithmetic
    y64, g64 = reference64(ref, theta, pts, gy)
    sl = block_slices(ref)

    def zero_blocks(j, n):
        return all(bool((g64[j, a:b] == 0).all()) for a, b in sl[:n])
    # what the reference itself says about these clouds (its ReLU passes no gradient at 0)
    assert zero_blocks(0, 9) and torch.allclose(g64[0, sl[9][0]:sl[9][1]], gy[0].double().sum(0))   # only db5 = sum grad_y
    assert zero_blocks(1, 5) and not zero_blocks(1, 6)                   # W1 b1 W2 b2 W3
    for j, (kind, l) in spec.items():
        if kind == "zero":
            assert zero_blocks(j, 2 * l + 1) and not zero_blocks(j, 2 * l + 2)       # ... W_l b_l W_{l+1}
    _CASES["exact"] = dict(B=B, N=N, theta=theta, pts=pts, gy=gy, y64=y64, g64=g64)
    return _CASES["exact"]


def test_exact_dead_and_zero_layers(ref):
    """Test 6a: in one 40 x 1300 batch, a cloud with b4 = -1e3 (only db5 = sum grad_y survives), one with b2 = -1e3 (W1 .. W3
    exactly 0), and for each hidden layer l a cloud with W_l = 0, b_l = 0: every pre-activation of that layer is exactly 0, the
    reference's ReLU passes no gradient at 0, so W_l, b_l, everything below and W_{l+1} are exactly 0.0 — which pins `>`
    against `>=` in each of the four masks (delta4's and the three of layer_dx).  The other 34 clouds are ordinary."""
    lib = _lib()
    case = _exact_case(ref)
    assert_forward(case, lib, "exact cases")
    assert_backward_all(ref, lib, case, "exact cases")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
def test_exact_zero_upstream_gradient_of_one_cloud(ref, fused):
    """Test 6b: grad_y == 0 for one cloud of a batch: its gradient is exactly zero and its neighbours' are, bit for bit, what
    they are when that cloud's grad_y is dense."""
    lib = _lib()
    case = make_case(ref, 40, 1300)
    theta_d, pts_d = padded(case["theta"]), case["pts"].cuda()
    run = (lambda gy: fused_backward(lib, theta_d, LD, pts_d, gy, calls=1)) if fused else \
          (lambda gy: layered(lib, theta_d, LD, pts_d, gy, calls=1)[1])
    dense = run(case["gy"].cuda())
    j = 7
    gy0 = case["gy"].clone()
    gy0[j] = 0.0
    got = run(gy0.cuda())
    assert torch.all(got[j] == 0), f"cloud {j}: max|grad| {got[j].abs().max().item():.3e} with a zero upstream gradient"
    keep = [i for i in range(40) if i != j]
    assert torch.equal(got[keep], dense[keep])


# ----------------------------------------------------------------------------------------------- 7: clouds do not leak
def test_permuting_clouds_permutes_outputs_bit_for_bit(ref):
    """Test 7: at 64 x 2048, permuting the clouds of theta / points / grad_y permutes y and grad_theta bit for bit (same B and
    N, hence the same launch), on both paths and both forward kernels."""
    lib = _lib()
    case = make_case(ref, 64, 2048)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(7))
    assert not torch.equal(perm, torch.arange(64))
    out = []
    for idx in (torch.arange(64), perm):
        theta_d, pts_d, gy_d = padded(case["theta"][idx]), case["pts"][idx].cuda(), case["gy"][idx].cuda()
        y1, y0 = fused_forward(lib, 1, theta_d, LD, pts_d), fused_forward(lib, 0, theta_d, LD, pts_d)
        gf = fused_backward(lib, theta_d, LD, pts_d, gy_d, calls=1).cpu()
        yl, gl = layered(lib, theta_d, LD, pts_d, gy_d, calls=1)
        out.append((y1, y0, gf, yl, gl.cpu()))
    for name, a, b in zip(("y f16 pipe", "y fp32", "grad fused", "y layered", "grad layered"), out[0], out[1]):
        assert torch.equal(a[perm], b), name


# ----------------------------------------------------------------------------------------------- 8: autograd route
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
@pytest.mark.parametrize("B,N", [(64, 2048), (40, 1300)])
def test_autograd_route_equals_c_abi_bit_for_bit(ref, B, N, fused):
    """Test 8: target_network_batched with theta.requires_grad_(): the gradient that reaches theta.grad is the C-ABI call's, bit
    for bit, when the upstream gradient is non-contiguous (the engine hands back the gradient of rec.permute(0, 2, 1))."""
    from hyperpocket_amd import ops
    from hyperpocket_amd.model.target_network import target_network_batched
    lib = _lib()
    case = make_case(ref, B, N)
    cfg = {"use_bias": True, "layer_out_channels": [32, 64, 128, 64]}
    theta = case["theta"].cuda().requires_grad_(True)
    pts_d = case["pts"].cuda()
    w = case["gy"].permute(0, 2, 1).contiguous().cuda()          # (B, 3, N): the layout the loss sees
    ops.FUSED_TARGET_NETWORK = fused
    try:
        y = target_network_batched(cfg, theta, pts_d)
        rec = y.permute(0, 2, 1)
        assert not w.permute(0, 2, 1).is_contiguous()
        rec.backward(w)
    finally:
        ops.FUSED_TARGET_NETWORK = True
    gy_d = w.permute(0, 2, 1).contiguous()
    if fused:
        want_y = fused_forward(lib, -1, theta.detach(), T, pts_d)
        want = fused_backward(lib, theta.detach(), T, pts_d, gy_d, calls=1)
    else:
        want_y, want = layered(lib, theta.detach(), T, pts_d, gy_d, calls=1)
    assert torch.equal(y.detach().cpu(), want_y)
    assert torch.equal(theta.grad, want)
    assert_blocks(ref, theta.grad, case["g64"], f"autograd route B={B} N={N} {'fused' if fused else 'layered'}")
