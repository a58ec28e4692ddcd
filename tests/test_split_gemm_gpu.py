"""GPU suite for the split-f16 ("piece format") GEMM kernels: csrc/conv_pp.hip (conv_pp_kernel<MODE,TN,WM> in its four
instances, pp_pack_kernel, pp_unpack_kernel) and csrc/conv_split.hip (conv_split_kernel<false>, split_rows_kernel,
absmax_kernel), through the stand-alone entry points hp_gemm_pp_* and hp_gemm_f16x2_*.

EXACT cases.  tests/split_gemm_law.py builds integer-valued operands for which every product, every partial sum in any
order, the along-k rescale and the store's re-split are exact (its header gives the construction,
tests/test_split_gemm_law_host.py proves the preconditions case by case without a GPU).  The expected result is the plain
fp64 product X W^T + b; values are compared with torch.equal, arg-max rows (the FIRST row of each 128-row tile that attains the
maximum) as integers.  One dropped, doubled or misplaced term, a wrong exponent on one k-block, a tile no workgroup visits, a
tie decided for the later row or a clamped row >= M that wins all change at least one output.  The tables:
  WALK_CASES      tile walks at K = 64: every kernel instance, tiles_n 1..8, grids of 1, 2, 4, multiples of 8 and the cap, walks
                  with and without a remainder, a single tile, M % 256 in {0, 1, 127, 128, 129, 255}
  K_CASES         K in {64, 128, 256, 512} with every admitted exponent-block width xcb (K .. 32: up to 16 blocks along k)
  EPI0_CASES      mode 0: bias alone, ReLU alone, both, an output block ReLU empties, a block whose maximum is a power of
                  two, outputs negative throughout
  EPI1_CASES      mode 1: group_rows 128, 256, 384 and the padded M; maxima planted on a tile's first row, its last row, two
                  rows at once and row M - 1 of a ragged tile
  F16X2_CASES     hp_gemm_f16x2_* (conv_split_kernel<false>)
Each case records the plan hp_gemm_pp_plan answers for it (the host suite proves the coverage from these records).

GUARDS on every case: C, cmax, cidx and the bias are views into larger buffers whose surroundings must keep their sentinel;
the workspace is exactly hp_gemm_pp_workspace_floats long, inside a buffer of 0xFF bytes (NaN) whose surroundings must stay
0xFF; a second run and a run on a side stream give the same bits.

The REAL-VALUED pass (REAL_CASES: rows spanning e^+-4, 10^5 between the two halves of K) bounds every element by a rounding
bound computed from the fp64 reference (split_gemm_law.real_bound), with x = a 2^e_a, y = w 2^e_w the scaled operands:
    splits        |x - hi - lo| <= 2^-22 |x| + 2^-38 max|block|   (hi: 2^-11 relative; lo: 2^-11 of the remainder, or half an
                  f16 subnormal step, 2^-25, against a block maximum >= 2^13), the same for y, through sum_k |a| dw + |w| da
    absent lo lo  2^-22 sum_k |a w|
    accumulation  3 K 2^-24 sum_k |a w|   (3 K fp32 additions, any order)
    store         2^-24 |v| (the bias fma) + 2^-22 |v| + 2^-38 max|output block| (the stored piece pair)
The accumulation term is a worst case over all orders and dominates the sum at large K, so the constant in front is measured,
not 1: split_gemm_law.simulate_f32 (the same formats, ONE fp32 summation order, on the CPU) reaches the share of the bound that
each of REAL_CASES records as law_ratio (asserted in the host suite), and the kernel is allowed twice that, the margin for
another order of the sum (the precedent of tests/test_gemm_paths_gpu.py).  Measured, error / bound (law | kernel on an MI355X):
    300 x 256 x 512, xcb 256          0.0100 | 0.0100
    300 x 128 x 64,  xcb 32, ReLU     0.2746 | 0.2746
    300 x 512 x 256, xcb 64           0.0699 | 0.0699
(the same to four digits: at the elements that come closest to the bound the error is the splits' and the stored pair's, which
the law and the kernel round alike; the summation order does not show there)."""
import ctypes

import numpy as np
import pytest
import torch

import split_gemm_law as law

pytestmark = pytest.mark.gpu

REAL_MARGIN = 2


def case(kind, mode, M, N, K=64, xcb=None, relu=0, plan=None, **kw):
    c = dict(kind=kind, mode=mode, M=M, N=N, K=K, xcb=xcb or K, relu=relu, plan=plan, **kw)
    c["seed"] = 1000003 * M + 1009 * N + 17 * K + 3 * c["xcb"] + mode
    return c


def case_id(c):
    extra = "".join(f"-{k}{c[k]}" for k in ("bias", "group_rows") if k in c)
    return f"{c['kind']}-m{c['mode']}-{c['M']}x{c['N']}x{c['K']}-cb{c['xcb']}-r{c['relu']}{extra}"


# plan = (bn, bm, tiles_n, tiles, workgroups, threads): what hp_gemm_pp_plan answers
WALK_CASES = [
    # mode 0, <0,1,1>: 128 x 128 tiles, 4 waves
    case("walk", 0, 127, 128, relu=1, plan=(128, 128, 1, 1, 1, 256)),
    case("walk", 0, 300, 128, xcb=32, plan=(128, 128, 1, 3, 1, 256)),
    case("walk", 0, 1153, 128, relu=1, plan=(128, 128, 1, 10, 8, 256)),
    case("walk", 0, 2048, 128, xcb=32, plan=(128, 128, 1, 16, 16, 256)),
    case("walk", 0, 65663, 128, relu=1, plan=(128, 128, 1, 513, 512, 256)),
    # mode 0, <0,2,2>: 256 x 256 tiles, 8 waves
    case("walk", 0, 255, 256, xcb=32, plan=(256, 256, 1, 1, 1, 512)),
    case("walk", 0, 513, 256, relu=1, plan=(256, 256, 1, 3, 1, 512)),
    case("walk", 0, 5120, 256, xcb=32, plan=(256, 256, 1, 20, 16, 512)),
    case("walk", 0, 384, 512, relu=1, plan=(256, 256, 2, 4, 2, 512)),
    case("walk", 0, 1100, 512, xcb=32, plan=(256, 256, 2, 10, 8, 512)),
    case("walk", 0, 200, 1024, relu=1, plan=(256, 256, 4, 4, 4, 512)),
    case("walk", 0, 700, 1024, xcb=32, plan=(256, 256, 4, 12, 8, 512)),
    case("walk", 0, 100, 2048, relu=1, plan=(256, 256, 8, 8, 8, 512)),
    case("walk", 0, 600, 2048, xcb=32, plan=(256, 256, 8, 24, 24, 512)),
    case("walk", 0, 8449, 2048, relu=1, plan=(256, 256, 8, 272, 256, 512)),
    # mode 1, <1,1,2>
    case("walk", 1, 129, 128, plan=(128, 256, 1, 1, 1, 512)),
    case("walk", 1, 700, 128, xcb=32, plan=(128, 256, 1, 3, 1, 512)),
    case("walk", 1, 2433, 128, plan=(128, 256, 1, 10, 8, 512)),
    # mode 1, <1,2,2>
    case("walk", 1, 255, 256, xcb=32, plan=(256, 256, 1, 1, 1, 512)),
    case("walk", 1, 383, 256, plan=(256, 256, 1, 2, 1, 512)),
    case("walk", 1, 5120, 256, xcb=32, plan=(256, 256, 1, 20, 16, 512)),
    case("walk", 1, 384, 512, plan=(256, 256, 2, 4, 2, 512)),
    case("walk", 1, 256, 1024, xcb=32, plan=(256, 256, 4, 4, 4, 512)),
    case("walk", 1, 511, 1024, plan=(256, 256, 4, 8, 8, 512)),
    case("walk", 1, 769, 1024, xcb=32, plan=(256, 256, 4, 16, 16, 512)),
    case("walk", 1, 600, 2048, plan=(256, 256, 8, 24, 24, 512)),
    case("walk", 1, 8449, 2048, xcb=32, plan=(256, 256, 8, 272, 256, 512)),
]

K_XCB = [(K, xcb) for K in (64, 128, 256, 512) for xcb in (512, 256, 128, 64, 32) if xcb <= K]
K_CASES = [case("k", mode, 300, (256, 128)[i % 2], K, xcb, relu=(i + mode) % 2,
                plan={(0, 128): (128, 128, 1, 3, 1, 256), (0, 256): (256, 256, 1, 2, 1, 512),
                      (1, 128): (128, 256, 1, 2, 1, 512), (1, 256): (256, 256, 1, 2, 1, 512)}[mode, (256, 128)[i % 2]])
           for i, (K, xcb) in enumerate(K_XCB) for mode in (0, 1)]

EPI0_CASES = [
    case("epi", 0, 300, 128, relu=0, bias="rand", plan=(128, 128, 1, 3, 1, 256)),
    case("epi", 0, 300, 512, relu=1, bias="zero", plan=(256, 256, 2, 4, 2, 512)),
    case("epi", 0, 300, 128, relu=1, bias="rand", plan=(128, 128, 1, 3, 1, 256)),
    case("epi", 0, 300, 512, relu=1, bias="neg0", plan=(256, 256, 2, 4, 2, 512)),      # ReLU empties column tile 0
    case("epi", 0, 300, 128, relu=0, bias="pow2", plan=(128, 128, 1, 3, 1, 256)),      # row tile 1 of X is zero: C = bias there
    case("epi", 0, 300, 256, relu=0, bias="neg", plan=(256, 256, 1, 2, 1, 512)),
]

PLANTS = [(0, None), (255, None), (261, None), (333, 261), (1188, None)]     # first row, last row, two at once, row M - 1
EPI1_CASES = [case("epi", 1, 1189, N, xcb=32, bigbits=12, plants=PLANTS, group_rows=g,
                   plan=(N, 256, 1, 5, 1, 512))
              for N, g in ((256, 128), (256, 256), (256, 384), (256, 1280), (128, 384), (128, 128))]

F16X2_CASES = [case("f16x2", 0, M, N, K, K, relu) for M, N, K, relu in
               ((1, 128, 32, 0), (127, 256, 96, 1), (128, 384, 512, 0), (129, 128, 512, 1), (300, 384, 96, 0), (300, 256, 32, 1))]

REAL_CASES = [case("real", 0, 300, 256, 512, 256, law_ratio=0.011), case("real", 0, 300, 128, 64, 32, relu=1, law_ratio=0.28),
              case("real", 0, 300, 512, 256, 64, law_ratio=0.07)]

EXACT_PP_CASES = WALK_CASES + K_CASES + EPI0_CASES + EPI1_CASES

SENT = -7777.0
PAD = 64


# ------------------------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope="module")
def lib():
    from hyperpocket_amd import _lib
    so = _lib.load_library()
    so.hp_gemm_pp_workspace_floats.restype = ctypes.c_long
    so.hp_gemm_f16x2_workspace_floats.restype = ctypes.c_long
    return so


def rc_of(fn_name, *args):
    """An entry point's return code (the library's `call` raises on non-zero)."""
    from hyperpocket_amd import _lib
    try:
        _lib.call(fn_name, *args)
        return 0
    except _lib.HipExtensionError as e:
        return int(str(e).rsplit(" ", 1)[1])


class Guarded:
    """A user buffer as a view into a larger one whose surroundings hold a sentinel."""

    def __init__(self, shape, dtype=torch.float32, sentinel=SENT, fill=None):
        n = int(np.prod(shape))
        self.sentinel = sentinel
        self.whole = torch.full((n + 2 * PAD,), sentinel, dtype=dtype, device="cuda")
        self.view = self.whole[PAD:PAD + n].view(*shape)
        if fill is not None:
            self.view.copy_(fill)

    def intact(self):
        return bool((self.whole[:PAD] == self.sentinel).all()) and bool((self.whole[-PAD:] == self.sentinel).all())


class Workspace:
    """Exactly `floats` floats inside a buffer of 0xFF bytes."""

    def __init__(self, floats):
        self.raw = torch.full((floats + 2 * PAD,), -1, dtype=torch.int32, device="cuda")
        self.ws = self.raw.view(torch.float32)[PAD:PAD + floats]
        self.bits = self.raw[PAD:PAD + floats]

    def intact(self):
        return bool((self.raw[:PAD] == -1).all()) and bool((self.raw[-PAD:] == -1).all())


def dev(ops):
    return {k: torch.from_numpy(v).cuda() for k, v in ops.items()}


def assert_plan(lib, c):
    out = (ctypes.c_int * 6)()
    assert lib.hp_gemm_pp_plan(ctypes.c_long(c["M"]), c["N"], c["mode"], 1, out) == 0
    assert tuple(out) == c["plan"] == law.plan(c["M"], c["N"], c["mode"]), case_id(c)


def first_rows(want, M, N, group_rows):
    """Per 128-row tile: column maxima of `want` (fp64) and the first row attaining each, reduced by group_rows."""
    t128 = (M + 127) // 128
    pad = torch.full((t128 * 128, N), float("-inf"), dtype=torch.float64, device="cuda")
    pad[:M] = want
    pad = pad.view(t128, 128, N)
    mx = pad.amax(dim=1)
    rows = torch.arange(t128 * 128, device="cuda").view(t128, 128, 1).expand(-1, -1, N)
    first = torch.where(pad == mx[:, None, :], rows, torch.full_like(rows, 1 << 40)).amin(dim=1)
    return mx, first % group_rows


class PpRun:
    """prepare once; run(mode) into fresh guarded buffers."""

    def __init__(self, lib, c, d):
        from hyperpocket_amd import _lib
        self._lib, self.c = _lib, c
        M, N, K = c["M"], c["N"], c["K"]
        self.W = Workspace(lib.hp_gemm_pp_workspace_floats(ctypes.c_long(M), N, K))
        self.bias = Guarded((N,), fill=d["b"], sentinel=float("nan"))
        self.bias_bits = self.bias.whole.view(torch.int32).clone()
        self.X, self.Wt = d["X"], d["W"]
        self.group_rows = c.get("group_rows", 128 * ((M + 127) // 128))
        _lib.call("hp_gemm_pp_prepare", ctypes.c_long(M), N, K, c["xcb"], self.X, self.Wt, self.W.ws, _lib.current_stream())

    def run(self, mode):
        _lib, c = self._lib, self.c
        M, N, K = c["M"], c["N"], c["K"]
        st = _lib.current_stream()
        _lib.call("hp_gemm_pp_run", ctypes.c_long(M), N, K, c["xcb"], self.bias.view, c["relu"] if mode == 0 else 0, mode,
                  self.group_rows if mode == 1 else 0, self.W.ws, st)
        if mode == 0:
            C = Guarded((M, N))
            _lib.call("hp_gemm_pp_unpack", ctypes.c_long(M), N, K, self.W.ws, C.view, st)
            return (C,)
        t128 = (M + 127) // 128
        cmax, cidx = Guarded((t128, N)), Guarded((t128, N), torch.int32, -7777)
        _lib.call("hp_gemm_pp_partials", ctypes.c_long(M), N, K, self.W.ws, cmax.view, cidx.view, st)
        return cmax, cidx

    def guards_intact(self):
        return self.W.intact() and torch.equal(self.bias.whole.view(torch.int32), self.bias_bits)


def same_bits(a, b):
    return all(torch.equal(x.whole.view(torch.int32), y.whole.view(torch.int32)) for x, y in zip(a, b))


def run_exact_pp(lib, c):
    assert_plan(lib, c)
    M, N, mode = c["M"], c["N"], c["mode"]
    d = dev(law.operands(c))
    want = d["X"].double() @ d["W"].double().t() + d["b"].double()
    r = PpRun(lib, c, d)
    out = r.run(mode)
    again = r.run(mode)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = r.run(mode)
    side.synchronize()
    torch.cuda.synchronize()
    if mode == 0:
        want = torch.relu(want) if c["relu"] else want
        assert torch.equal(out[0].view.double(), want), case_id(c)
    else:
        mx, first = first_rows(want, M, N, r.group_rows)
        assert torch.equal(out[0].view.double(), mx), case_id(c)
        assert torch.equal(out[1].view.long(), first), case_id(c)
        # (equal to the first row below M of its own tile, reduced by group_rows: in its tile, never a clamped row >= M)
        assert int(out[1].view.min()) >= 0 and int(out[1].view.max()) < min(r.group_rows, M), case_id(c)
    assert same_bits(out, again) and same_bits(out, other), case_id(c)
    assert all(g.intact() for g in out + again + other) and r.guards_intact(), case_id(c)
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("c", WALK_CASES, ids=case_id)
def test_tile_walks_are_exact(lib, c):
    run_exact_pp(lib, c)


@pytest.mark.parametrize("c", K_CASES, ids=case_id)
def test_every_k_and_exponent_block_width_is_exact(lib, c):
    run_exact_pp(lib, c)


@pytest.mark.parametrize("c", EPI0_CASES, ids=case_id)
def test_store_epilogues_are_exact(lib, c):
    run_exact_pp(lib, c)


@pytest.mark.parametrize("c", EPI1_CASES, ids=case_id)
def test_colmax_epilogue_names_the_first_row_and_reduces_it_by_group_rows(lib, c):
    cidx = run_exact_pp(lib, c)[1].view.cpu().numpy()
    # the planted rows are what the call reports (the host suite proves that they are the maxima)
    live = np.abs(law.operands(c)["W"]).max(axis=1) > 0
    for row in (0, 255, 261, 1188):
        assert (cidx[row // 128][live] == row % c["group_rows"]).all(), (case_id(c), row)


# ------------------------------------------------------------------------------------------------- the format kernels
def ws_images(c, W):
    """The packed operands inside a hp_gemm_pp workspace (the layout csrc/conv_pp.hip states above hp_gemm_pp_prepare):
    [X lines: M K | X exponents: 16 per 128-row tile | weight exponents: N | W lines: N K | ...]."""
    M, N, K = c["M"], c["N"], c["K"]
    t128 = (M + 127) // 128
    bits = W.bits.cpu().numpy()
    o = 0
    xl = bits[o:o + M * K].view(np.uint16).reshape(M, 2 * K); o += M * K
    xe = bits[o:o + t128 * (K // c["xcb"])].reshape(t128, -1); o += t128 * 16
    we = bits[o:o + N]; o += N
    wl = bits[o:o + N * K].view(np.uint16).reshape(N, 2 * K); o += N * K
    return xl, xe, we, wl, o


FORMAT_CASES = [case("fmt", 0, 300, 128, 96, 32), case("fmt", 0, 129, 256, 96, 96), case("fmt", 0, 300, 128, 512, 32),
                case("fmt", 0, 257, 128, 160, 32), case("fmt", 0, 128, 256, 64, 64)]


@pytest.mark.parametrize("kind", ["integer", "real"])
@pytest.mark.parametrize("c", FORMAT_CASES, ids=case_id)
def test_prepare_writes_the_laws_images_and_unpack_restores_integer_operands(lib, c, kind):
    """pp_pack_kernel and split_rows_kernel against the law's restatement, bit for bit on integer views: exponents, hi and lo
    pieces, line layout; K = 32 * odd included (prepare admits it, the P-format run does not), a row of zeros in W, a zero block
    in X.  For the integer operands the law's unpack of the kernel's image is X (and W) again."""
    from hyperpocket_amd import _lib
    M, N, K = c["M"], c["N"], c["K"]
    ops = law.operands(c) if kind == "integer" else law.real_operands(c)
    if kind == "real":
        ops["W"][5] = 0
        ops["X"][128:256, :c["xcb"]] = 0
    d = dev(ops)
    W = Workspace(lib.hp_gemm_pp_workspace_floats(ctypes.c_long(M), N, K))
    _lib.call("hp_gemm_pp_prepare", ctypes.c_long(M), N, K, c["xcb"], d["X"], d["W"], W.ws, _lib.current_stream())
    torch.cuda.synchronize()
    xl, xe, we, wl, end = ws_images(c, W)
    ah, al, aexp = law.pack_act(ops["X"], c["xcb"])
    wh, wlo, wexp = law.pack_rows(ops["W"])
    assert np.array_equal(xe, aexp) and np.array_equal(we, wexp)
    assert np.array_equal(xl, law.lines(ah, al)) and np.array_equal(wl, law.lines(wh, wlo))
    assert W.intact() and bool((W.bits[end:] == -1).all())             # prepare writes nothing behind the operands
    if kind == "integer":
        h, l = law.unlines(xl, K)
        e = np.repeat(np.repeat(xe, 128, axis=0)[:M], c["xcb"], axis=1)
        assert np.array_equal(law.unpack(h, l, e).view(np.int32), ops["X"].view(np.int32))
        h, l = law.unlines(wl, K)
        got = law.unpack(h, l, we[:, None])
        assert np.array_equal(got, ops["W"]) and not np.signbit(got[5]).any()


@pytest.mark.parametrize("c", [case("fmt", 0, 300, 128, 64, 32), case("fmt", 0, 129, 512, 128, 128, relu=1)], ids=case_id)
def test_store_and_unpack_kernels_write_the_laws_image_of_real_valued_results(lib, c):
    """Mode 0's stored piece pairs are a fixed point of the format: what hp_gemm_pp_unpack returns, packed again by the law
    under the stored block exponent and unpacked, is the same fp32 bits (compared on integer views), and the stored
    exponents are block_exp of the blocks' maxima."""
    M, N, K = c["M"], c["N"], c["K"]
    ops = law.real_operands(c)
    r = PpRun(lib, c, dev(ops))
    C = r.run(0)[0].view.cpu().numpy()
    t128, bn = (M + 127) // 128, law.pp_bn(N)
    end = ws_images(c, r.W)[4]
    cexp = r.W.bits[end + M * N:end + M * N + t128 * 16].cpu().numpy()[:t128 * (N // bn)].reshape(t128, N // bn)
    for t in range(t128):
        for j in range(N // bn):
            blk = C[t * 128:(t + 1) * 128, j * bn:(j + 1) * bn]
            e, m = int(cexp[t, j]), np.abs(blk).max()
            # (the exponent comes from the maximum BEFORE the store's rounding: one more where that rounds up to a power of two)
            assert e == int(law.block_exp(m)) or (e == int(law.block_exp(m)) + 1 and np.frexp(m)[0] == 0.5), (t, j)
            assert np.array_equal(law.unpack(*law.split(blk, e), e).view(np.int32), blk.view(np.int32)), (t, j)


# -------------------------------------------------------------------------------------------------------------- f16x2
@pytest.mark.parametrize("c", F16X2_CASES, ids=case_id)
def test_f16x2_gemm_is_exact(lib, c):
    from hyperpocket_amd import _lib
    M, N, K = c["M"], c["N"], c["K"]
    d = dev(law.operands(c))
    want = d["X"].double() @ d["W"].double().t() + d["b"].double()
    want = torch.relu(want) if c["relu"] else want
    W = Workspace(lib.hp_gemm_f16x2_workspace_floats(ctypes.c_long(M), N, K))
    bias = Guarded((N,), fill=d["b"], sentinel=float("nan"))
    bias_bits = bias.whole.view(torch.int32).clone()
    _lib.call("hp_gemm_f16x2_prepare", ctypes.c_long(M), N, K, d["X"], d["W"], W.ws, _lib.current_stream())
    outs = []
    side = torch.cuda.Stream()
    for stream in (None, None, side):
        C = Guarded((M, N))
        if stream is None:
            _lib.call("hp_gemm_f16x2_run", ctypes.c_long(M), N, K, d["X"], bias.view, C.view, c["relu"], W.ws, _lib.current_stream())
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                _lib.call("hp_gemm_f16x2_run", ctypes.c_long(M), N, K, d["X"], bias.view, C.view, c["relu"], W.ws,
                          _lib.current_stream())
            stream.synchronize()
        outs.append(C)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view.double(), want), case_id(c)
    assert all(torch.equal(outs[0].whole.view(torch.int32), o.whole.view(torch.int32)) and o.intact() for o in outs)
    assert W.intact() and torch.equal(bias.whole.view(torch.int32), bias_bits)


# ----------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("M,N,K", [(200, 384, 64), (200, 128, 32), (200, 256, 96)])
@pytest.mark.parametrize("mode", [0, 1])
def test_shapes_the_launch_refuses_leave_everything_untouched(lib, M, N, K, mode):
    """N = 384 (no whole 256-column tiles) and K = 32, 96 (an odd number of k-tiles) pass the argument checks of prepare and
    run; the launch refuses them: non-zero, and C, cmax and cidx inside the workspace keep their bytes."""
    c = case("refuse", mode, M, N, K, K)
    d = dev(law.operands(c))
    W = Workspace(lib.hp_gemm_pp_workspace_floats(ctypes.c_long(M), N, K))
    st = torch.cuda.current_stream().cuda_stream
    args = lambda: (ctypes.c_long(M), N, K, K)
    assert rc_of("hp_gemm_pp_prepare", *args(), d["X"], d["W"], W.ws, ctypes.c_void_p(st)) == 0
    torch.cuda.synchronize()
    before = W.raw.clone()
    assert rc_of("hp_gemm_pp_run", *args(), d["b"], 0, mode, 256, W.ws, ctypes.c_void_p(st)) != 0
    torch.cuda.synchronize()
    end = ws_images(c, W)[4]
    assert torch.equal(W.raw, before) and bool((W.bits[end:] == -1).all()) and W.intact()
    if N == 384:
        assert lib.hp_gemm_pp_plan(ctypes.c_long(M), N, mode, 1, (ctypes.c_int * 6)()) != 0


def test_argument_checks_refuse(lib):
    M, N, K = 200, 128, 64
    d = dev(law.operands(case("refuse", 0, M, N, K)))
    W = Workspace(lib.hp_gemm_pp_workspace_floats(ctypes.c_long(M), N, 512))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = ctypes.c_long
    prep = lambda M=M, N=N, K=K, xcb=K, X=d["X"], Wt=d["W"], ws=W.ws: rc_of("hp_gemm_pp_prepare", L(M), N, K, xcb, X, Wt, ws, st)
    run = lambda M=M, N=N, K=K, xcb=K, b=d["b"], mode=0, g=0, ws=W.ws: rc_of("hp_gemm_pp_run", L(M), N, K, xcb, b, 0, mode, g, ws, st)
    assert prep() == 0 and run() == 0 and run(mode=1, g=256) == 0
    assert prep(xcb=48) != 0 and run(xcb=48) != 0                       # xcb does not divide K / is no multiple of 32
    assert prep(K=96, xcb=64) != 0 and run(K=96, xcb=64) != 0
    assert prep(K=128, xcb=16) != 0 and run(K=128, xcb=16) != 0
    assert prep(K=1024, xcb=32) != 0                                    # K > 512 (and K / xcb > 16)
    assert prep(X=None) != 0 and prep(Wt=None) != 0 and prep(ws=None) != 0
    assert run(b=None) != 0 and run(ws=None) != 0
    assert run(mode=1, g=0) != 0 and run(mode=2) != 0 and run(mode=-1) != 0
    assert prep(M=0) != 0 and run(M=0) != 0 and prep(N=100) != 0 and run(N=100) != 0
    C = torch.empty(M, N, device="cuda")
    assert rc_of("hp_gemm_pp_unpack", L(M), N, K, None, C, st) != 0 and rc_of("hp_gemm_pp_unpack", L(M), N, K, W.ws, None, st) != 0
    assert rc_of("hp_gemm_pp_partials", L(M), N, K, W.ws, None, C, st) != 0
    torch.cuda.synchronize()
    assert W.intact()


# ------------------------------------------------------------------------------------------------------ real-valued pass
@pytest.mark.parametrize("c", REAL_CASES, ids=case_id)
def test_real_valued_results_stay_inside_the_rounding_bound(lib, c):
    ops = law.real_operands(c)
    d = dev(ops)
    want = d["X"].double() @ d["W"].double().t() + d["b"].double()
    want = torch.relu(want) if c["relu"] else want
    C = PpRun(lib, c, d).run(0)[0].view
    bound = torch.from_numpy(law.real_bound(c, ops, want.cpu().numpy())).cuda()
    ratio = ((C.double() - want).abs() / bound).max().item()
    print(f"{case_id(c)}: kernel error / bound = {ratio:.4f} (allowed {REAL_MARGIN * c['law_ratio']:.4f})")
    assert ratio <= REAL_MARGIN * c["law_ratio"], (case_id(c), ratio)


# ------------------------------------------------------------------------------------------------------ the real layers
# (B, Np): B Np = 128, 384, 5 * 256 + 128, and 258 tiles of 128 rows — more than one pass of the planned grids (asserted below)
ENC_SHAPES = [(1, 128), (3, 128), (1, 1408), (2, 16512)]
ENC_SEEDS = (11, 12)                    # the two encoders of a pair have different weights
ENC_CLOUD_SEED = 5
ENC_LAYERS = ((128, 0), (256, 0), (512, 0), (512, 1))       # (N, mode) of layers 2..5


def _enc_params(seed, is_vae):
    """The encoder's flat parameter list with the law's integer conv stack; the heads behind the pool are zeroed (their
    outputs are not this file's subject and stay finite)."""
    import encoder_law as elaw
    p = elaw.make_params(seed, 128, is_vae)
    Ws, bs = law.encoder_weights(seed)
    for l in range(5):
        assert tuple(p[l].shape) == Ws[l].shape
        p[l], p[5 + l] = torch.from_numpy(Ws[l]), torch.from_numpy(bs[l])
    for i in range(10, len(p), 2):
        p[i] = torch.zeros_like(p[i])
    return p


def _assert_layers_exact(side, x, seed, tag):
    B, Np = x.shape[:2]
    Ws, bs = law.encoder_weights(seed)
    g, arg = side.g.clone(), side.argidx.clone()
    hs = side.hidden()
    h = x.cuda().double().view(B * Np, 3)
    for l in range(5):
        h = h @ torch.from_numpy(Ws[l]).cuda().double().t() + torch.from_numpy(bs[l]).cuda().double()
        if l < 4:
            h = torch.relu(h)
            assert torch.equal(hs[l].double(), h), (tag, "h%d" % (l + 1))
    h5 = h.view(B, Np, 512)
    mx = h5.amax(dim=1)
    rows = torch.arange(Np, device="cuda").view(1, Np, 1).expand(B, Np, 512)
    first = torch.where(h5 == mx[:, None, :], rows, torch.full_like(rows, 1 << 40)).amin(dim=1)
    assert torch.equal(g.double(), mx), (tag, "g")
    assert torch.equal(arg.long(), first), (tag, "argidx")


@pytest.mark.parametrize("presplit", [1, 0], ids=["pformat", "split_f32"])
@pytest.mark.parametrize("n", [1, 2], ids=["single", "pair"])
@pytest.mark.parametrize("B,Np", ENC_SHAPES, ids=lambda v: str(v))
def test_encoder_layers_are_exact_on_integer_clouds(lib, B, Np, n, presplit):
    """conv1_pp_kernel / conv1_kernel, layers 2..4 (store) and layer 5 with the fused max-pool, as hp_encoder_forward and
    hp_encoder_forward_pair launch them: h1..h4, g and argidx against the fp64 chain and the first-point rule, exactly.
    presplit = 0 runs conv_split_kernel<false> and conv_split_kernel<true> (fp32 activations, split in the consumer)."""
    import encoder_law as elaw
    from hyperpocket_amd import _lib, ops
    x = torch.from_numpy(law.encoder_cloud(B, Np, ENC_CLOUD_SEED))
    with elaw.switches(1, presplit):                                     # (restores both switches on exit)
        plan = ops.encoder_plan(B, Np, 128, (True, False)[:n] if n == 2 else (False,))
        assert plan["conv"] == ("pformat" if presplit else "split_f32") and plan["pool_fused"] and plan["tile_rows"] == 128
        if presplit:
            out = (ctypes.c_int * 6)()
            passes = []
            for N, mode in ENC_LAYERS:
                assert lib.hp_gemm_pp_plan(ctypes.c_long(B * Np), N, mode, n, out) == 0
                passes.append(out[3] > out[4])
            assert all(passes) or B * Np < 32768        # the large shape: every layer's workgroups walk several tiles
        if n == 1:
            s = elaw.Side(B, Np, 128, x, _enc_params(ENC_SEEDS[0], False), None).forward()
            torch.cuda.synchronize()
            _assert_layers_exact(s, x, ENC_SEEDS[0], "single")
            return
        latent = elaw._filled(elaw.fresh, (B, 256))
        eps = torch.zeros(B, 128)
        sides = [elaw.Side(B, Np, 128, x, _enc_params(ENC_SEEDS[z], z == 0), eps if z == 0 else None, latent=latent) for z in (0, 1)]
        io = (ops._EncoderIO * 2)(sides[0].io(), sides[1].io())
        _lib.call("hp_encoder_forward_pair", B, Np, 128, io, _lib.current_stream(latent.device))
        torch.cuda.synchronize()
        for z in (0, 1):
            _assert_layers_exact(sides[z], x, ENC_SEEDS[z], f"pair, encoder {z}")
