"""GPU suite for the general fp32 GEMM family (csrc/gemm.hip: hp_gemm_f32, hp_colsum_f32): every tile x staging-loader
instance, every epilogue, the fused column max, both split-K reduce paths, the device-side sizes and the column sums, each
against an fp64 reference of the same contraction.

Exact inputs are the main tool: operands, bias and addend are non-zero integers from {-4..-1, 1..4} held as fp32.  With
K <= 2048 every partial sum stays below 2^24, so every fp32 summation order and every split gives the same exact value, the
fp64 reference is exact too, and the comparison is torch.equal: one dropped, duplicated or misplaced term fails.  Mask entries
come from {-1, 0, 1}, so `> 0` is tested at 0.

Guards on every case: operands, mask and addend are views with padded rows whose padding holds NaN, and a NaN band follows each
buffer; `out` is a padded view of a buffer pre-filled with a sentinel, and the whole buffer — padding and the band behind it
included — is compared with what it must hold afterwards.  Each case records the (tile, mode) it runs and asserts it against
hp_gemm_plan; tests/test_gemm_plan_host.py proves from these tables alone (no GPU) that together they reach all 4 tiles x 7
loader instances.

A second, smaller pass uses real-valued operands and bounds every element by a rounding bound computed from the reference:
    |got - want| <= 2 (K + ksplit + 4) 2^-24 (sum_k |a_ik b_kj| + |bias_j| + |add_ij|)
(a chain of K + ksplit + 3 fp32 additions; the factor 2 covers an MFMA step that rounds product and sum separately).  No
tolerance relative to a tensor's maximum appears in this file."""
import types
import zlib

import numpy as np
import pytest
import torch

NAN = float("nan")
SENTINEL = -12345.0
GUARD = 64                          # floats behind every buffer
TILE_ROWS = (128, 128, 64, 64)      # rows of tile 0: 128x32, 1: 128x128, 2: 64x128, 3: 64x64
MODE_OF = {(0, 0): 0, (1, 0): 1, (2, 0): 2, (0, 1): 3, (1, 1): 4, (2, 1): 3, (0, 2): 0, (1, 2): 7, (2, 2): 8}


def case(tile, mode, M, N, K, batch, am=1, bm=1, **opts):
    """One table row.  am / bm: how A / B is stored — 0 transposed (lanes run along i / j), 1 K-contiguous with a row stride
    that is a multiple of 4 floats and a 16-byte-aligned base, 2 K-contiguous with an odd row stride ("2s") or a base offset by
    one float ("2o"); which of the two is `a2` / `b2`.  opts: bias ("batched": sBiasz = N, "shared": sBiasz = 0), relu, mask,
    add, pads (extra floats per row of out, mask, add), ksplit, rowsum, colmax (group_rows), dyn ("rows" | "k", count), real."""
    c = dict(tile=tile, mode=mode, M=M, N=N, K=K, batch=batch, am=am, bm=bm, a2="s", b2="o", bias=None, relu=False, mask=False,
             add=False, pads=(0, 0, 0), ksplit=1, rowsum=False, colmax=None, dyn=None, real=False)
    assert set(opts) <= set(c), opts
    c.update(opts)
    return c


def case_id(c):
    s = f"t{c['tile']}m{c['mode']}-{c['M']}x{c['N']}x{c['K']}b{c['batch']}-a{c['am']}b{c['bm']}"
    for k in ("bias", "colmax", "dyn"):
        if c[k] is not None:
            s += f"-{k}{c[k]}".replace(" ", "").replace("'", "")
    for k in ("relu", "mask", "add", "rowsum", "real"):
        if c[k]:
            s += "-" + k
    if c["ksplit"] > 1:
        s += f"-ks{c['ksplit']}"
    if any(c["pads"]):
        s += "-ld" + "_".join(map(str, c["pads"]))
    return s


# base shape (M, N, K, batch) per tile: ragged last row tile and ragged last column tile everywhere; tile 1 needs K % 16 == 0
# and >= 384 workgroups (2 x 2 tiles x 96), tile 2 >= 512 workgroups of 64x128 (2 x 2 x 128)
BASE = {0: (130, 19, 37, 3), 1: (130, 130, 48, 96), 2: (100, 200, 37, 128), 3: (100, 130, 70, 2)}
# smaller shapes of the same tiles for the tables that carry full-size epilogue operands
SMALL = {0: (130, 19, 37, 3), 1: (130, 130, 16, 96), 2: (70, 130, 21, 128), 3: (100, 130, 70, 2)}

# a. every tile x every operand-loader pair: 36 cases, all 28 kernels.  K = 37 on row stride 40 is loader 1 with a K tail;
# the loader-2 operands alternate between an odd row stride and an offset base from tile to tile
LOADER_CASES = [case(t, MODE_OF[am, bm], *BASE[t], am=am, bm=bm, a2="so"[t % 2], b2="os"[t % 2])
                for t in range(4) for bm in range(3) for am in range(3)]
# the smallest problems, and K = 0, which must give exactly the epilogue of zero
LOADER_CASES += [case(0, 8, 1, 1, 1, 1, am=2, bm=2), case(3, 8, 1, 33, 1, 1, am=2, bm=2),
                 case(3, 4, 70, 70, 0, 1, bias="shared", relu=True), case(3, 0, 70, 70, 0, 2, am=0, bm=0, bias="batched", add=True)]

# b. epilogues on every tile: each flag alone, all together, batched bias both ways, ldc / ldmask / ldadd each != N and
# different from one another
EPILOGUE_CASES = []
for _t in range(4):
    _s = SMALL[_t]
    EPILOGUE_CASES += [case(_t, 4, *_s, bias="batched"), case(_t, 4, *_s, bias="shared"), case(_t, 4, *_s, relu=True),
                       case(_t, 4, *_s, mask=True), case(_t, 4, *_s, add=True), case(_t, 4, *_s, pads=(5, 0, 0)),
                       case(_t, 4, *_s, mask=True, pads=(0, 3, 0)), case(_t, 4, *_s, add=True, pads=(0, 0, 1)),
                       case(_t, 4, *_s, bias="batched", add=True, relu=True, mask=True),
                       case(_t, MODE_OF[_t % 3, (_t + 1) % 3], *_s, am=_t % 3, bm=(_t + 1) % 3, bias="shared", add=True, relu=True,
                            mask=True, pads=(3, 1, 6))]

# c. ROWSUM without split-K, through each loader of A on each tile.  M is never a multiple of the tile rows; K is no multiple
# of the k-tile depth except on tile 1, which only takes whole k-tiles
ROWSUM_CASES = [case(t, MODE_OF[ab, ab], *BASE[t], am=ab, bm=ab, rowsum=True) for t in range(4) for ab in range(3)]


def _colmax_shape(tile, groups, group_tiles, batch):
    """M = groups x group_rows with group_rows = group_tiles x tile rows; N ragged and wide enough for the tile's workgroup
    threshold at this M and batch (the encoder's conv5 + max-pool launches are that wide)."""
    rows = TILE_ROWS[tile]
    M = groups * group_tiles * rows
    tiles_m = M // rows
    if tile == 0:
        return M, 19, 5, rows * group_tiles
    if tile == 3:
        return M, 70, 5, rows * group_tiles
    need, K = (384, 16) if tile == 1 else (512, 21)
    tiles_n = -(-need // (tiles_m * batch))
    return M, (tiles_n - 1) * 128 + 5, K, rows * group_tiles


# d. COLMAX on every tile: group_rows = tile rows (3 groups) and 2 x tile rows (2 groups), batch 1 and 2, with and without bias
COLMAX_CASES = []
for _t in range(4):
    for _gt, _groups in ((1, 3), (2, 2)):
        for _b in (1, 2):
            for _bias in (None, "batched"):
                _M, _N, _K, _g = _colmax_shape(_t, _groups, _gt, _b)
                COLMAX_CASES.append(case(_t, 4 if _bias else 0, _M, _N, _K, _b, am=1 if _bias else 0, bm=1 if _bias else 0,
                                         bias=_bias, colmax=_g))

# e. split-K: what each row reaches is in the right-hand column
SPLITK_CASES = []
for _row, _scalar in [(case(1, 4, 130, 132, 256, 12, ksplit=8), False),                    # float4 reduce, tile 1
                      (case(1, 0, 130, 131, 256, 12, am=0, bm=0, ksplit=8), True),         # scalar reduce, tile 1
                      (case(3, 8, 77, 65, 1500, 1, am=2, bm=2, ksplit=23), True),          # 16 + 4 + 3 slabs of slab_sum
                      (case(3, 4, 77, 65, 736, 1, ksplit=23), True),                       # the same loops, no slab empty
                      (case(2, 7, 70, 130, 200, 32, am=1, bm=2, ksplit=16), True),         # tile 2, one 16-slab round
                      (case(0, 0, 200, 32, 70, 2, am=0, bm=0, ksplit=5), False),           # tile 0, float4 reduce of 5 slabs
                      (case(3, 4, 48, 40, 40, 1, ksplit=13), True)]:                       # splits 2..12 are empty
    SPLITK_CASES.append(dict(_row, bias="batched", relu=True))
    SPLITK_CASES.append(dict(_row, bias="batched", relu=True, rowsum=True))
    if _scalar:
        SPLITK_CASES.append(dict(_row, bias="shared", add=True, relu=True, mask=True, rowsum=True, pads=(3, 2, 5)))

# f. device-side sizes.  dyn_rows: tile 1 is chosen for a third of the static bound (Meff = 133: 2 x 2 x 96 workgroups); counts
# 0, 1, one more than a tile boundary, the bound and a value above it.  dyn_k (with split-K and ROWSUM; a device-side K bars
# tile 1): counts 0, 1, around one k-tile, the bound and above
DYN_CASES = [case(1, 4, 400, 130, 32, 96, dyn=("rows", n)) for n in (0, 1, 129, 400, 450)]
DYN_CASES += [case(3, 2, 150, 70, 40, 2, am=2, bm=0, mask=True, dyn=("rows", n)) for n in (0, 1, 65, 150, 200)]
DYN_CASES += [case(2, MODE_OF[ab, ab], 130, 130, 256, 16, am=ab, bm=ab, ksplit=23, rowsum=True, dyn=("k", n))
              for ab in (0, 1) for n in (0, 1, 31, 32, 33, 256, 300)]

# real-valued operands: one case per tile, plain and split-K (the same tile at half the batch and two splits, or three)
REAL_CASES = [case(0, 4, *BASE[0], real=True, bias="batched", add=True),
              case(0, 4, *BASE[0], real=True, bias="batched", add=True, ksplit=3),
              case(1, 4, *BASE[1], real=True, bias="batched", add=True),
              case(1, 4, 130, 130, 48, 48, real=True, bias="batched", add=True, ksplit=2),
              case(2, 4, *BASE[2], real=True, bias="batched", add=True),
              case(2, 4, 100, 200, 37, 64, real=True, bias="batched", add=True, ksplit=2),
              case(3, 4, *BASE[3], real=True, bias="batched", add=True),
              case(3, 4, *BASE[3], real=True, bias="batched", add=True, ksplit=3)]

GEMM_TABLES = {"loaders": LOADER_CASES, "epilogues": EPILOGUE_CASES, "rowsum": ROWSUM_CASES, "colmax": COLMAX_CASES,
               "splitk": SPLITK_CASES, "dyn": DYN_CASES, "real": REAL_CASES}

# g. hp_colsum_f32: (M, N) around the 512-row threshold of the slabbed form and the 64-column workgroups
COLSUM_SHAPES = [(1, 1), (130, 70), (511, 64), (512, 65), (4100, 200)]


# ----------------------------------------------------------------------------------------------------------- inputs
def ints(g, *shape):
    """non-zero integers from {-4..-1, 1..4} as fp32"""
    return (torch.randint(1, 5, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


class Padded:
    """vals (b, R, W) laid out with row stride ld at `off` floats into a buffer that holds `fill` everywhere else: in the
    padding columns, in front of the base and in a band of GUARD floats behind the last row."""

    def __init__(self, vals, ld, off=0, fill=NAN):
        self.shape, self.ld, self.off = tuple(vals.shape), ld, off
        self.flat = torch.full((off + vals.shape[0] * vals.shape[1] * ld + GUARD,), fill)
        self.view().copy_(vals)

    def to(self, dev):
        self.flat = self.flat.to(dev)
        return self

    def view(self):
        b, R, W = self.shape
        return self.flat[self.off:self.off + b * R * self.ld].view(b, R, self.ld)[:, :, :W]


def operand(vals, kind, variant):
    """vals: the logical (b, rows, K) operand.  Stored as case() describes kind / variant."""
    K = vals.shape[2]
    if kind == 0:
        return Padded(vals.transpose(1, 2), vals.shape[1] + 3)
    if kind == 1:
        return Padded(vals, (K // 4 + 1) * 4)
    if variant == "s":
        return Padded(vals, K + 1 + K % 2)                 # odd: 1 or 3 (mod 4)
    return Padded(vals, (K // 4 + 1) * 4, off=1)


def make(c, dev):
    """The tensors of a case on `dev` and the arguments ops.gemm / ops.gemm_plan take.  Nothing here computes a result."""
    g = torch.Generator().manual_seed(zlib.crc32(repr(sorted((k, v) for k, v in c.items() if k != "dyn")).encode()))
    draw = (lambda *s: torch.randn(*s, generator=g)) if c["real"] else (lambda *s: ints(g, *s))
    b, M, N, K = c["batch"], c["M"], c["N"], c["K"]
    x = types.SimpleNamespace(a=draw(b, M, K), w=draw(b, N, K), bias=None, add=None, mask=None, out=None, count=None)
    a_st, w_st = x.a.clone(), x.w.clone()
    kw = dict(trans_a=c["am"] == 0, trans_b=c["bm"] != 0, relu=c["relu"], ksplit=c["ksplit"], rowsum=c["rowsum"])
    if c["dyn"]:
        kind, x.count = c["dyn"]
        n = torch.tensor([x.count], dtype=torch.int32).to(dev)
        if kind == "rows":
            a_st[:, x.count:] = NAN                        # rows at or above the count must not be read
            kw["dyn_rows"] = n
        else:
            a_st[:, :, x.count:] = NAN
            w_st[:, :, x.count:] = NAN
            kw["dyn_k"] = n
    x.A = operand(a_st, c["am"], c["a2"]).to(dev)
    x.B = operand(w_st, c["bm"], c["b2"]).to(dev)
    if c["bias"]:
        x.bias = draw(b, N) if c["bias"] == "batched" else draw(N)
        kw["bias"] = x.bias.to(dev)
    if c["mask"]:
        x.mask = torch.randint(-1, 2, (b, M, N), generator=g).float()
        x.Mask = Padded(x.mask, N + c["pads"][1]).to(dev)
        kw["mask"] = x.Mask.view()
    if c["add"]:
        x.add = draw(b, M, N)
        x.Add = Padded(x.add, N + c["pads"][2]).to(dev)
        kw["add"] = x.Add.view()
    if c["colmax"] is None:
        x.out = Padded(torch.full((b, M, N), SENTINEL), N + c["pads"][0], fill=SENTINEL).to(dev)
        kw["out"] = x.out.view()
    else:
        kw["colmax"] = c["colmax"]
    x.kw = kw
    return x


def reference(c, x):
    """fp64 on the CPU, the documented epilogue order: bias, add, ReLU, mask.  Returns (C, sum of magnitudes, row sums)."""
    a, w = x.a.double(), x.w.double()
    if c["dyn"] and c["dyn"][0] == "k":
        a, w = a[:, :, :x.count], w[:, :, :x.count]
    v = torch.bmm(a, w.transpose(1, 2))
    mag = torch.bmm(a.abs(), w.abs().transpose(1, 2))
    if x.bias is not None:
        bias = x.bias.double() if x.bias.dim() == 2 else x.bias.double().expand(c["batch"], -1)
        v = v + bias[:, None, :]
        mag = mag + bias.abs()[:, None, :]
    if x.add is not None:
        v = v + x.add.double()
        mag = mag + x.add.double().abs()
    if c["relu"]:
        v = torch.relu(v)
    if x.mask is not None:
        v = torch.where(x.mask > 0, v, torch.zeros_like(v))
    return v, mag, a.sum(2)


def run_exact(c):
    from hyperpocket_amd import ops
    x = make(c, "cuda")
    A, B = x.A.view(), x.B.view()
    assert ops.gemm_plan(A, B, **x.kw) == (c["tile"], c["mode"])
    res = ops.gemm(A, B, **x.kw)
    want, _, rsum = reference(c, x)
    rows = min(c["M"], x.count) if c["dyn"] and c["dyn"][0] == "rows" else c["M"]
    expect = Padded(torch.full(x.out.shape, SENTINEL), x.out.ld, fill=SENTINEL)
    expect.view()[:, :rows] = want.float()[:, :rows]
    got = x.out.flat.cpu()
    assert torch.equal(got, expect.flat), f"{(got != expect.flat).sum().item()} of {got.numel()} floats differ"
    if c["rowsum"]:
        assert torch.equal(res[1].cpu(), rsum.float())
    if c["ksplit"] > 1:                                    # ordered, atomic-free reduce: run to run identical
        x.kw["out"].fill_(SENTINEL)
        again = ops.gemm(A, B, **x.kw)
        assert torch.equal(x.out.flat.cpu(), got)
        if c["rowsum"]:
            assert torch.equal(again[1], res[1])


# ----------------------------------------------------------------------------------------------------------- tests
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", LOADER_CASES, ids=case_id)
def test_every_tile_and_loader_pair_is_exact(c):
    run_exact(c)


@pytest.mark.parametrize("c", EPILOGUE_CASES, ids=case_id)
def test_epilogues_are_exact_on_every_tile(c):
    run_exact(c)


@pytest.mark.parametrize("c", ROWSUM_CASES, ids=case_id)
def test_rowsum_is_exact_on_every_tile(c):
    run_exact(c)


@pytest.mark.parametrize("c", SPLITK_CASES, ids=case_id)
def test_splitk_reduce_paths_are_exact_and_repeatable(c):
    run_exact(c)


@pytest.mark.parametrize("c", DYN_CASES, ids=case_id)
def test_device_side_sizes_are_exact(c):
    run_exact(c)


def check_colmax(c, x, cmax, cidx):
    """cmax exact; cidx the FIRST row attaining the max within its row tile, modulo group_rows."""
    want = reference(c, x)[0].float().numpy()
    rows, b, N = TILE_ROWS[c["tile"]], c["batch"], c["N"]
    tiles = want.reshape(b, c["M"] // rows, rows, N)
    first = tiles.argmax(2)                                # numpy: the first occurrence
    assert cmax.shape == (b, c["M"] // rows, N) and cidx.dtype == torch.int32
    assert np.array_equal(cmax.cpu().numpy(), tiles.max(2))
    want_idx = (first + (np.arange(c["M"] // rows) * rows)[None, :, None]) % c["colmax"]
    assert np.array_equal(cidx.cpu().numpy(), want_idx)
    return tiles, first


@pytest.mark.parametrize("c", COLMAX_CASES, ids=case_id)
def test_colmax_is_exact_and_keeps_the_first_row(c):
    from hyperpocket_amd import ops
    x = make(c, "cuda")
    assert ops.gemm_plan(x.A.view(), x.B.view(), **x.kw) == (c["tile"], c["mode"])
    cmax, cidx = ops.gemm(x.A.view(), x.B.view(), **x.kw)
    tiles, _ = check_colmax(c, x, cmax, cidx)
    ties = (tiles == tiles.max(2, keepdims=True)).sum(2)
    assert (ties > 1).any()                                # integer inputs: the tie rule is exercised in every case


# Rows of one 64-row block at which a column's maximum is attained.  In every tile a wave row is 32 rows, and within it the lower
# lane half owns the rows with (row % 8) < 4, the upper half the others.  The sets put the first maximum in either half and in
# either wave row, with later maxima in the other half and the other wave row.
TIE_ROWS = [(6, 9, 37, 40), (1, 6, 33, 38), (37, 40), (33, 38), (12, 16, 63), (31, 32), (0, 63), (27, 28, 59, 60)]


@pytest.mark.parametrize("c", [case(3, 4, 128, 70, 8, 1, colmax=64), case(0, 4, 256, 19, 8, 2, colmax=128),
                               case(3, 0, 128, 70, 8, 2, am=0, bm=0, colmax=128, bias="batched")], ids=case_id)
def test_colmax_ties_across_lane_halves_and_wave_rows(c):
    """Column j of C follows pattern j % 8: A(i, p) is 4 at the pattern's tie rows and below 4 elsewhere, B(j, :) selects one
    pattern.  Later 64-row blocks rotate the patterns; in the 128-row tiles the maximum then also recurs in wave rows 2 and 3."""
    from hyperpocket_amd import ops
    x = make(c, "cuda")
    g = torch.Generator().manual_seed(5)
    x.a = torch.randint(-4, 4, x.a.shape, generator=g).float()
    for blk in range(c["M"] // 64):
        for p, rows in enumerate(TIE_ROWS):
            x.a[:, [64 * blk + r for r in rows], (p + 3 * blk) % 8] = 4.0
    x.w = torch.zeros_like(x.w)
    x.w[:, torch.arange(c["N"]), torch.arange(c["N"]) % 8] = 1.0
    x.A = operand(x.a, c["am"], c["a2"]).to("cuda")
    x.B = operand(x.w, c["bm"], c["b2"]).to("cuda")
    assert ops.gemm_plan(x.A.view(), x.B.view(), **x.kw) == (c["tile"], c["mode"])
    cmax, cidx = ops.gemm(x.A.view(), x.B.view(), **x.kw)
    tiles, first = check_colmax(c, x, cmax, cidx)
    within = first % 64
    upper = (within % 8) >= 4
    assert upper.any() and (~upper).any() and (within >= 32).any() and (within < 32).any()


@pytest.mark.parametrize("c", REAL_CASES, ids=case_id)
def test_real_valued_operands_stay_within_the_rounding_bound(c):
    from hyperpocket_amd import ops
    x = make(c, "cuda")
    assert ops.gemm_plan(x.A.view(), x.B.view(), **x.kw) == (c["tile"], c["mode"])
    ops.gemm(x.A.view(), x.B.view(), **x.kw)
    want, mag, _ = reference(c, x)
    got = x.out.view().cpu().double()
    bound = 2.0 * (c["K"] + c["ksplit"] + 4) * 2.0 ** -24 * mag
    worst = ((got - want).abs() / bound).max().item()
    print(f"{case_id(c)}: worst error / bound = {worst:.3f}")
    assert torch.isfinite(got).all() and worst <= 1.0
    expect = Padded(torch.full(x.out.shape, SENTINEL), x.out.ld, fill=SENTINEL)
    expect.view().copy_(got.float())
    assert torch.equal(x.out.flat.cpu(), expect.flat)      # nothing written outside C


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("M,N", COLSUM_SHAPES)
def test_colsum_is_exact(M, N, batch):
    """One slab (no workspace, or fewer than 512 rows) against the slabbed form + finish kernel, with and without mask (the
    unmasked loop is the unrolled one), dense and row-padded X; the slabbed form twice."""
    from hyperpocket_amd import ops
    g = torch.Generator().manual_seed(M * 31 + N + batch)
    xs, mk = ints(g, batch, M, N), torch.randint(-1, 2, (batch, M, N), generator=g).float()
    want = {False: xs.double().sum(1).float(), True: torch.where(mk > 0, xs, torch.zeros_like(xs)).double().sum(1).float()}
    for pad in (0, 3):
        X, Mk = Padded(xs, N + pad).to("cuda"), Padded(mk, N + (2 * pad) // 3).to("cuda")
        for masked in (False, True):
            for use_ws in (True, False):
                got = ops.colsum(X.view(), mask=Mk.view() if masked else None, use_ws=use_ws)
                assert torch.equal(got.cpu(), want[masked]), (pad, masked, use_ws)
                if use_ws:
                    assert torch.equal(ops.colsum(X.view(), mask=Mk.view() if masked else None, use_ws=True), got)
    got2 = ops.colsum(Padded(xs[0:1], N).to("cuda").view()[0])          # the 2-D form
    assert torch.equal(got2.cpu(), want[False][0])
