"""The reference the halo-plan tests compare against: plain numpy on host arrays in the reference layout [8,8,8,n_blocks(,K)],
flattened in Fortran order. pack is flat[index], unpack is flat[index] = message - nothing here knows how the library stores a field
(block order, block-major layout, 32-byte sectors).

Everything is compared as 32-bit words (`bits`): the kernels under test copy words, so field contents are arbitrary bit patterns -
signed zeros, subnormals, infinities, NaNs with payloads - and a value that went through arithmetic, or two elements that changed
places, always shows. No tolerance anywhere."""
import numpy as np

# bit patterns every random fill contains: +0, -0, smallest / largest subnormal of either sign, +Inf, -Inf, quiet and signalling NaNs
# with payloads, of either sign
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x007FFFFF, 0x80000001, 0x7F800000, 0xFF800000,
                     0x7FC00000, 0x7FC12345, 0xFFC0BEEF, 0x7F800001, 0xFFBFFFFF, 0x7FFFFFFF], dtype=np.uint32)
SENTINEL = np.uint32(0x7FA5DEAD)       # a signalling NaN with a payload: what an element nobody may write holds


def n_elements(n_blocks: int, K: int) -> int:
    return 512 * n_blocks * K


def shape(n_blocks: int, K: int):
    return (8, 8, 8, n_blocks) + ((K,) if K > 1 else ())


def offset(n_blocks: int, k, b, cell):
    """element offset of component k, block b (reference order), cell x + 8 y + 64 z"""
    return (np.asarray(k, dtype=np.int64) * n_blocks + np.asarray(b, dtype=np.int64)) * 512 + np.asarray(cell, dtype=np.int64)


def bits(a: np.ndarray) -> np.ndarray:
    """the array's 32-bit words, flattened in Fortran order (= by element offset)"""
    a = np.asarray(a)
    assert a.dtype.itemsize == 4
    return a.reshape(-1, order="F").view(np.uint32)


def as_field(words: np.ndarray, n_blocks: int, K: int) -> np.ndarray:
    """words by element offset -> a Float32 array of the level's shape (Fortran order), same bits"""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    assert words.size == n_elements(n_blocks, K)
    return words.view(np.float32).reshape(shape(n_blocks, K), order="F")


def random_words(n: int, seed: int) -> np.ndarray:
    """n random 32-bit patterns; every eighth or so is one of SPECIALS (all of them occur once n >= 8 * len(SPECIALS))"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if n:
        where = rng.permutation(n)[: max(n // 8, min(n, SPECIALS.size))]
        w[where] = SPECIALS[np.arange(where.size) % SPECIALS.size]
    return w


def offset_words(n: int, tag: int = 0) -> np.ndarray:
    """every element distinct: its own offset as an integer bit pattern (tag in the top four bits tells fields apart), so that a
    failure can say which element landed where"""
    assert n < (1 << 28) and 0 <= tag < 16
    return (np.arange(n, dtype=np.uint64) | (np.uint64(tag) << np.uint64(28))).astype(np.uint32)


def pack(field_words: np.ndarray, index: np.ndarray) -> np.ndarray:
    return field_words[np.asarray(index, dtype=np.int64)]


def unpack(field_words: np.ndarray, index: np.ndarray, message: np.ndarray) -> np.ndarray:
    """a new array: field with flat[index] = message (index must not name an element twice: the result would depend on the order)"""
    index = np.asarray(index, dtype=np.int64)
    assert np.unique(index).size == index.size, "a receive list names an element twice"
    out = field_words.copy()
    out[index] = message
    return out


def first_difference(got: np.ndarray, want: np.ndarray) -> str:
    """for assertion messages: where two word arrays differ first and, for an offset fill, which element's value sits there"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shapes {got.shape} != {want.shape}"
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return "identical"
    i = int(bad[0])
    return f"{bad.size} of {got.size} words differ, first at {i}: got 0x{int(got[i]):08X}, want 0x{int(want[i]):08X}"
