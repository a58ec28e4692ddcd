"""CPU suite for the pair form of the EMD: hp_emd_pairs' argument checks (they return before any HIP call, so nothing reaches a
GPU) and the chunking rule of utils/evaluation/emd_pairs.py, which is host arithmetic over the library's size queries."""
import ctypes
import importlib.util
import os

import pytest

from conftest import PKG_DIR

c_int, c_long, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = ctypes.CDLL(mod.build(verbose=False))
    so.hp_emd_pairs.restype = c_int
    so.hp_emd_pairs.argtypes = [c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p]
    for name in ("hp_approxmatch_workspace_floats", "hp_emd_partials_floats"):
        getattr(so, name).restype = c_long
        getattr(so, name).argtypes = [c_int, c_int, c_int]
    return so


def test_invalid_arguments_are_rejected_without_a_gpu(lib):
    buf = (ctypes.c_float * 4)()          # a non-NULL host address: a call that gets past the checks would fail differently
    some = ctypes.cast(buf, c_void_p)

    def call(na=2, n=8, nb=2, m=8, pairs=1, A=some, B=some, ab=some, temp=some, ws=some, part=some, cost=some):
        return lib.hp_emd_pairs(na, n, A, nb, m, B, pairs, ab, temp, ws, part, cost, None)

    for kw in [dict(na=0), dict(na=-1), dict(nb=0), dict(nb=-3), dict(n=0), dict(n=-1), dict(m=0), dict(m=-8), dict(pairs=-1),
               dict(pairs=65536), dict(pairs=1 << 20)]:
        assert call(**kw) == -1, kw
    for name in ("A", "B", "ab", "temp", "ws", "part", "cost"):            # NULL buffers with pairs > 0
        assert call(**{name: None}) == -1, name
    assert lib.hp_emd_pairs(2, 8, None, 2, 8, None, 65536, None, None, None, None, None, None) == -1
    # nothing to do: no pointer is touched, whatever it holds
    assert lib.hp_emd_pairs(2, 8, None, 2, 8, None, 0, None, None, None, None, None, None) == 0
    assert call(pairs=0, n=100, m=37) == 0


@pytest.mark.parametrize("n,m", [(2048, 2048), (100, 37)])
@pytest.mark.parametrize("budget", [1 << 20, 1 << 30, 1 << 40])
def test_chunk_is_the_largest_that_fits_the_budget(lib, n, m, budget):
    from hyperpocket_amd.utils.evaluation.emd_pairs import MAX_CHUNK, emd_pairs_buffer_floats, emd_pairs_chunk

    def bytes_of(c):          # from the library's queries directly, not through the module under test
        return 4 * (c * (n + m) * 2 + lib.hp_approxmatch_workspace_floats(c, n, m) + lib.hp_emd_partials_floats(c, n, m))

    chunk = emd_pairs_chunk(n, m, budget)
    assert 4 * sum(emd_pairs_buffer_floats(chunk, n, m)) == bytes_of(chunk)
    assert 1 <= chunk <= MAX_CHUNK == 65535
    print(f"n={n} m={m} budget 2^{budget.bit_length() - 1}: chunk {chunk}, {bytes_of(chunk)} bytes, one pair {bytes_of(1)} bytes")
    if bytes_of(1) > budget:
        assert chunk == 1          # one pair is always run
    else:
        assert bytes_of(chunk) <= budget
        assert chunk == MAX_CHUNK or bytes_of(chunk + 1) > budget


def test_chunk_floor_cap_and_interior(lib):
    """The three outcomes of the rule: a budget below one pair's buffers still runs one pair, a budget above 65 535 pairs' stops at
    the cap, and in between the chunk moves with the budget by exactly the pairs that fit."""
    from hyperpocket_amd.utils.evaluation.emd_pairs import emd_pairs_buffer_floats, emd_pairs_chunk
    for n, m in ((2048, 2048), (100, 37)):
        one = 4 * sum(emd_pairs_buffer_floats(1, n, m))
        assert emd_pairs_chunk(n, m, 0) == 1 and emd_pairs_chunk(n, m, one - 4) == 1 and emd_pairs_chunk(n, m, one) == 1
        assert emd_pairs_chunk(n, m, 1 << 40) == 65535
        three = 4 * sum(emd_pairs_buffer_floats(3, n, m))
        assert emd_pairs_chunk(n, m, three) == 3 and emd_pairs_chunk(n, m, three - 4) == 2
    assert 1 < emd_pairs_chunk(2048, 2048, 1 << 30) < 65535 and 1 < emd_pairs_chunk(100, 37, 1 << 20) < 65535
    with pytest.raises(ValueError):
        emd_pairs_chunk(0, 8, 1 << 20)
