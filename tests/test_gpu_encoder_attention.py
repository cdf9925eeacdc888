"""The encoder's unmasked ragged attention kernels alone (fl_op_encoder_attention) against fp64 numpy softmax attention.

Bounds, both measured on the CPU, never on the kernel:
  fp32  10 * e32, e32 = max |numpy float32 run - fp64| of the same attention on the same inputs
  bf16  1.5 * (max error of the same attention done in numpy with the probabilities rounded to bf16 before P V and the output rounded
        to bf16, as the kernel does) + 1e-3: outputs are bf16-rounded, and 2^-8 relative is the format's own step
One case fills the rows of the neighbouring sequences' K and V with +-30: a read across a sequence boundary then shows as a gross
error, not as noise."""
import numpy as np
import pytest

import bert_ref as R

pytestmark = pytest.mark.gpu

RAGGED = [1, 17, 64, 3, 33, 16]
SETS = [[1], [31], [32], [33], [64], [65], [160], RAGGED]


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def rb(a):
    return R.bf16_bits_to_f32(R.f32_to_bf16_bits(a))


def attention_ref(q, k, v, lengths, H, dtype=np.float64, round_p=False):
    out, r0 = np.empty(q.shape, dtype=np.float64), 0
    d = q.shape[1] // H
    for n in lengths:
        sl = slice(r0, r0 + n)
        if not round_p:
            out[sl] = R.attention(q[sl].astype(dtype), k[sl].astype(dtype), v[sl].astype(dtype), H)
        else:                                       # the kernel's rounding points: p = exp(s - max) -> bf16 for P V, l from the unrounded p, out -> bf16
            for hh in range(H):
                c = slice(hh * d, (hh + 1) * d)
                s = q[sl, c].astype(np.float64) @ k[sl, c].astype(np.float64).T / np.sqrt(d)
                p = np.exp(s - s.max(axis=-1, keepdims=True))
                out[sl, c] = rb((rb(p.astype(np.float32)).astype(np.float64) @ v[sl, c].astype(np.float64) / p.sum(axis=-1, keepdims=True)).astype(np.float32))
        r0 += n
    return out


_CASES = {}


def case(lengths, H, d, seed=11):
    """inputs (bf16-rounded float32) and the fp64 / float32 / bf16-emulated references, computed once"""
    key = (tuple(lengths), H, d, seed)
    if key not in _CASES:
        rs = np.random.RandomState(seed + 7 * H + d + sum(lengths))
        q, k, v = (rb(rs.standard_normal((sum(lengths), H * d)).astype(np.float32)) for _ in range(3))
        r64 = attention_ref(q, k, v, lengths, H)
        e32 = np.abs(attention_ref(q, k, v, lengths, H, dtype=np.float32) - r64).max()
        e16 = np.abs(attention_ref(q, k, v, lengths, H, round_p=True) - r64).max()
        _CASES[key] = (q, k, v, r64, e32, e16)
    return _CASES[key]


def run(fa, q, k, v, lengths, H, d, dtype):
    if dtype == "bf16":
        q, k, v = (R.f32_to_bf16_bits(a) for a in (q, k, v))
    return fa.op_encoder_attention(q, k, v, lengths, H, d)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("lengths", SETS, ids=lambda l: "x".join(map(str, l)))
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("d", [32, 64])
def test_attention_against_fp64(fa, d, H, lengths, dtype):
    q, k, v, r64, e32, e16 = case(lengths, H, d)
    out = run(fa, q, k, v, lengths, H, d, dtype)
    err = np.abs(out - r64).max()
    bound = 10 * e32 if dtype == "f32" else 1.5 * e16 + 1e-3
    print("\nd=%d H=%d %s %s: e32 %.3e, bf16-emulation error %.3e, achieved %.3e (bound %.3e)" % (d, H, lengths, dtype, e32, e16, err, bound))
    assert np.isfinite(out).all()
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [32, 64])
def test_neighbouring_sequences_are_never_read(fa, d, dtype):
    """Sequences 1 and 4 of the ragged set keep their values; K and V of every other sequence are +-30.  Their outputs must be what
    they are with ordinary neighbours -- bit for bit -- and within the bound of the reference."""
    H = 3
    q, k, v, r64, e32, e16 = case(RAGGED, H, d)
    offs = np.concatenate([[0], np.cumsum(RAGGED)])
    k2, v2 = k.copy(), v.copy()
    rs = np.random.RandomState(3)
    for s in (0, 2, 3, 5):
        sl = slice(offs[s], offs[s + 1])
        k2[sl] = 30.0 * rs.choice([-1.0, 1.0], size=k2[sl].shape)
        v2[sl] = 30.0 * rs.choice([-1.0, 1.0], size=v2[sl].shape)
    a, b = run(fa, q, k, v, RAGGED, H, d, dtype), run(fa, q, k2, v2, RAGGED, H, d, dtype)
    bound = 10 * e32 if dtype == "f32" else 1.5 * e16 + 1e-3
    for s in (1, 4):
        sl = slice(offs[s], offs[s + 1])
        assert np.array_equal(a[sl], b[sl]), s
        assert np.abs(b[sl] - r64[sl]).max() <= bound
    assert np.isfinite(b).all()
