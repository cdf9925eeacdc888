"""The K/V prefix copy kernel alone (fl_op_kv_copy, k_kvcopy.hip), byte-exact against numpy: the first `width` bytes of every source
row arrive in the same row of the destination, and every other byte of the destination -- the rest of each row up to its pitch --
keeps the sentinel it was filled with.

Widths cover the 16-byte chunking (below one chunk, one chunk exactly, one chunk and a 2-byte tail, the 14-byte tail, many chunks
with and without a tail); the pitches differ in both directions, are equal, and equal the width (no gap between rows: the last row
ends where the buffer ends); the row counts are one, fewer than a wave's lanes, several workgroups, and more rows than any grid has
threads (the grid-stride loop)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDTHS = [2, 14, 16, 18, 62, 64, 66, 4094, 4096]
ROWS = [1, 3, 257, 70001]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1, "no MI355X visible"
    return fastllm_amd


def pattern(rows, pitch, seed):
    """[rows, pitch] bytes that differ from row to row and never equal the sentinel (a block of random bytes repeated with a period
    that is no multiple of any pitch used here)."""
    block = np.random.RandomState(seed).randint(0, 255, size=65521, dtype=np.uint8)
    block[block == SENTINEL] = 0x5A
    return np.resize(block, rows * pitch).reshape(rows, pitch)


def pitch_cases(width):
    """(src pitch, dst pitch): (64, 128) and (128, 64) where the width fits them, else the same two relations above the width; equal
    pitches; pitch == width where the width is a multiple of 16."""
    up = (width + 15) // 16 * 16
    cases = [(64, 128), (128, 64)] if width <= 64 else [(up + 64, up + 128), (up + 128, up + 64)]
    cases.append((up + 16, up + 16))
    if width % 16 == 0:
        cases.append((width, width))
    return cases


def check(fa, rows, width, sp, dp, seed):
    src = pattern(rows, sp, seed)
    dst = np.full((rows, dp), SENTINEL, np.uint8)
    got = fa.op_kv_copy(src, dst, width)
    want = dst.copy()
    want[:, :width] = src[:, :width]
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("rows %d width %d pitches %d -> %d: %d wrong bytes, first at row %d byte %d (got 0x%02x, want 0x%02x)"
                             % (rows, width, sp, dp, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("width", WIDTHS)
def test_copy_is_byte_exact_and_touches_nothing_else(fa, width, rows):
    for i, (sp, dp) in enumerate(pitch_cases(width)):
        check(fa, rows, width, sp, dp, seed=1000 * width + 10 * rows + i)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("es", [2, 4])
def test_shapes_of_a_two_layer_cache(fa, d, es):
    """K (and row-major V) and transposed V of a two-layer, two-kv-head cache: source capacity 96, destinations 40 (seq_alloc 64), 96
    and 200 (seq_alloc 224); n = 1, 7, 33 cached positions."""
    L, Hkv, sa_src = 2, 2, 96
    for sa_dst in (64, 96, 224):
        for n in (1, 7, 33):
            check(fa, L * Hkv, n * d * es, sa_src * d * es, sa_dst * d * es, seed=n + d)            # K: [L][Hkv][seq_alloc][d]
            check(fa, L * Hkv * d, n * es, sa_src * es, sa_dst * es, seed=n + d + 1)                # V^T: [L][Hkv][d][seq_alloc]
