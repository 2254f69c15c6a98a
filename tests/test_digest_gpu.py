"""GPU: ops.state_digest / dcfp_state_digest_u64 (csrc/digest.hip) against its numpy restatement in uint64
arithmetic: d0 = sum w_i, d1 = sum (base + i + 1) * w_i mod 2^64 over the buffer read as 32-bit words.  Exact equality
everywhere - integer sums have no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from dcfp_amd import _lib, ops

pytestmark = pytest.mark.gpu

CHUNK, BLOCKS = _lib.DIGEST_CHUNK, _lib.DIGEST_MAX_BLOCKS
MASK = (1 << 64) - 1


def restate(words, base=0):
    w = words.astype(np.uint64)
    idx = np.arange(1, w.size + 1, dtype=np.uint64) + np.uint64(base & MASK)
    with np.errstate(over="ignore"):
        return int(w.sum(dtype=np.uint64)), int((idx * w).sum(dtype=np.uint64))


def words_on(cuda, n, seed, pad=0):
    g = torch.Generator(device=cuda).manual_seed(seed)
    t = torch.randint(-2 ** 31, 2 ** 31, (n + pad,), dtype=torch.int32, device=cuda, generator=g)
    return t


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


# one word past a whole number of chunks for one block, for several, and for every block of the capped grid twice over
LENGTHS = [0, 1, 3, 4, 5, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1, 2 * BLOCKS * CHUNK + 1]


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(cuda, n):
    t = words_on(cuda, n, 100 + n % 97)
    got = ops.state_digest(t)
    assert got == restate(as_u32(t)), n
    assert ops.state_digest(t) == got                     # two calls, the same pair
    if n == 0:
        assert got == (0, 0)


def test_arena_sized_buffer(cuda):
    n = 65 * 1000 * 1000 + 7
    t = words_on(cuda, n, 7)
    got = ops.state_digest(t, base=3)
    assert got == restate(as_u32(t), 3)
    assert ops.state_digest(t, base=3) == got


@pytest.mark.parametrize("start", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 6, 1025, 2 * CHUNK + 5])
def test_slices_that_are_only_4_byte_aligned(cuda, start, n):
    whole = words_on(cuda, n, 11 * start + n % 13, pad=8)
    t = whole[start:start + n]
    assert t.data_ptr() % 16 == 4 * start
    assert ops.state_digest(t, base=9) == restate(as_u32(whole)[start:start + n], 9)


@pytest.mark.parametrize("base", [0, 2 ** 32 - 5, 2 ** 40])
def test_index_base(cuda, base):
    """b + i + 1 crosses 2^32 inside the buffer for base = 2^32 - 5 (at i = 4), in the head, the body and a second chunk."""
    for start, n in ((0, 3), (0, CHUNK + 77), (3, 2 * CHUNK + 1)):
        whole = words_on(cuda, n, 5 + start, pad=4)
        t = whole[start:start + n]
        assert ops.state_digest(t, base=base) == restate(as_u32(whole)[start:start + n], base), (start, n)


def test_floats_are_read_as_bits(cuda):
    bits = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000001, 0x807FFFFF,
                     0x3F800000, 0xBF800000], dtype=np.uint32)
    bits = np.tile(bits, 150)[:1499]
    t = torch.from_numpy(bits.view(np.float32).copy()).to(cuda)
    assert t.dtype == torch.float32
    got = ops.state_digest(t)
    assert got == restate(bits)
    zeros = torch.zeros(64, device=cuda)
    minus = zeros.clone()
    minus[17] = -0.0
    assert bool((zeros == minus).all())                   # equal as floats ...
    assert ops.state_digest(zeros) == (0, 0)
    assert ops.state_digest(minus) == (0x80000000, 18 * 0x80000000)      # ... different as state


def test_a_swap_of_two_different_words_changes_d1(cuda):
    t = words_on(cuda, 5000, 21)
    a = ops.state_digest(t)
    s = t.clone()
    s[[7, 4500]] = t[[4500, 7]]
    b = ops.state_digest(s)
    assert int(t[7]) != int(t[4500]) and a[0] == b[0] and a[1] != b[1]


@pytest.mark.parametrize("na,nb", [(0, 9), (5, 0), (3, 1030), (CHUNK + 1, 2 * CHUNK + 3)])
def test_pieces_add_up(cuda, na, nb):
    t = words_on(cuda, na + nb, 31 + na % 7)
    whole = ops.state_digest(t, base=12)
    a = ops.state_digest(t[:na], base=12)
    b = ops.state_digest(t[na:], base=12 + na)
    assert whole == ((a[0] + b[0]) & MASK, (a[1] + b[1]) & MASK)


def test_int32_and_float32_views_agree_and_other_tensors_are_refused(cuda):
    t = words_on(cuda, 777, 41)
    assert ops.state_digest(t) == ops.state_digest(t.view(torch.float32))
    with pytest.raises(RuntimeError):
        ops.state_digest(t.cpu())
    with pytest.raises(RuntimeError):
        ops.state_digest(t.to(torch.int64))
    with pytest.raises(RuntimeError):
        ops.state_digest(t[::2])
    with pytest.raises(ValueError):
        ops.state_digest(t, base=-1)


def test_bad_arguments_launch_nothing(cuda):
    L = _lib.lib()
    n = 3 * CHUNK
    t = words_on(cuda, n, 51)
    need = L.dcfp_state_digest_workspace_bytes(n)
    assert need == 3 * 16 and L.dcfp_state_digest_workspace_bytes(0) == 0
    assert L.dcfp_state_digest_workspace_bytes(1 << 40) == BLOCKS * 16
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    out = torch.full((2,), 77, dtype=torch.int64, device=cuda)
    p = lambda x: C.c_void_p(x.data_ptr())
    assert L.dcfp_state_digest_u64(None, n, 0, p(ws), need, p(out), None) == _lib.E_BADDESC
    assert L.dcfp_state_digest_u64(p(t), n, 0, p(ws), need - 1, p(out), None) == _lib.E_WORKSPACE
    assert L.dcfp_state_digest_u64(p(t), n, 0, None, need, p(out), None) == _lib.E_WORKSPACE
    assert L.dcfp_state_digest_u64(p(t), n, 0, p(ws), need, None, None) == _lib.E_BADDESC
    assert L.dcfp_state_digest_u64(C.c_void_p(t.data_ptr() + 2), 8, 0, p(ws), need, p(out), None) == _lib.E_BADDESC
    torch.cuda.synchronize()
    assert out.tolist() == [77, 77] and int(ws.sum()) == 0          # nothing was launched
    assert L.dcfp_state_digest_u64(p(t), n, 0, p(ws), need, p(out), None) == 0
    torch.cuda.synchronize()
    assert tuple(v & MASK for v in out.tolist()) == restate(as_u32(t))
    assert L.dcfp_state_digest_u64(None, 0, 5, None, 0, p(out), None) == 0      # n = 0: (0, 0), nothing read
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0]
