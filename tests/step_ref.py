"""Token selection's step state and the row-moving launches restated on the host: the yardstick of test_gpu_select_rows_ops.py and
test_gpu_move_rows_ops.py.  Plain Python / numpy index formulas, no device code; every comparison against it is equality.

    selection       out_tokens[step] = tok;  token = tok;  done = 1 if eos >= 0 and tok == eos (never cleared);
                    then pos, len, step += advance (uint32).  Selection goes on after `done`: the host stops a decode loop.
    ArgMax          the LAST maximal index (logit_rules_ref.argmax_last); over a candidate list: the largest value, ties -> the larger
                    index, over the first `count` entries
    log-prob slot   the record of a selection goes to slot step_after - advance, and nowhere when that slot >= cap

Sampled tokens and the contents of a log-prob record are not re-derived here: the tests take them from op_sample / op_logprobs, which
have their own tests against the oracle.  This file also holds the inputs both the CPU "teeth" tests (test_step_ref.py) and the GPU
tests use, so that what the former show about the data holds for the latter."""
import numpy as np

from logit_rules_ref import argmax_last

FILL = np.uint32(0xFFFFFFFF)          # a device word no launch wrote
U32 = 1 << 32
STATE_FIELDS = ("token", "pos", "len", "step", "eos", "done", "error", "call0")

# index pairs that land in different lanes, waves and passes of the 1024-lane ArgMax: the row's two ends; lanes 63 | 64 of the scalar
# walk and of the 16-byte walk (elements 255 | 256); the wrap of the 1024 lanes (1023 | 1024, and 4095 | 4096 in 16-byte units); and the
# second trip of the eight-load loop (32767 | 32768)
TIE_PAIRS = ((63, 64), (255, 256), (1023, 1024), (4095, 4096), (32767, 32768))


def argmax_first(y):
    return int(np.flatnonzero(y == y.max())[0])


def tie_rows(V, seed=0):
    """float32 [R, V]: row 0 ties its first and last element, the next ones tie each pair of TIE_PAIRS that fits V, and the last one
    ties three elements spread over the row; everything else lies well below."""
    rng = np.random.default_rng(seed + V)
    groups = [(0, V - 1)] + [p for p in TIE_PAIRS if p[1] < V] + [(1, V // 2, V - 2)]
    rows = rng.uniform(-4.0, 4.0, size=(len(groups), V)).astype(np.float32)
    for r, g in enumerate(groups):
        rows[r, list(g)] = np.float32(9.0 + 0.25 * r)
    return rows


def cand_argmax(values, indices, count=None):
    """the consumer of an lm_head launch's candidate list: the largest value of the first `count` entries, ties -> the larger index"""
    n = len(values) if count is None else int(count)
    v, ix = np.asarray(values[:n], dtype=np.float32), np.asarray(indices[:n], dtype=np.int64)
    return int(ix[v == v.max()].max())


def cand_argmin_index(values, indices, count=None):
    """the wrong tie rule: the SMALLER index among the maxima"""
    n = len(values) if count is None else int(count)
    v, ix = np.asarray(values[:n], dtype=np.float32), np.asarray(indices[:n], dtype=np.int64)
    return int(ix[v == v.max()].min())


def chunk_candidates(row, chunk):
    """the list an lm_head launch leaves for `row`: one (value, index) per chunk of `chunk` rows, each the chunk's argmax_last"""
    row = np.asarray(row, dtype=np.float32)
    idx = [c0 + argmax_last(row[c0:c0 + chunk]) for c0 in range(0, row.size, chunk)]
    return row[idx].copy(), np.asarray(idx, dtype=np.int32)


def state(token=0, pos=0, len=0, step=0, eos=-1, done=0, error=0, call0=0):
    return dict(token=token, pos=pos, len=len, step=step, eos=eos, done=done, error=error, call0=call0)


def select_step(st, out_tokens, tok, advance):
    """one selection launch on a state dict and the member's out_tokens buffer (both updated in place)"""
    out_tokens[st["step"]] = np.uint32(tok)
    st["token"] = int(tok)
    if st["eos"] >= 0 and int(tok) == st["eos"]:
        st["done"] = 1
    if advance:
        for f in ("pos", "len", "step"):
            st[f] = (st[f] + 1) % U32
    return st


def select_run(st0, tokens, advance, out_cap):
    """n launches selecting tokens[0..n): (the final state, the out_tokens buffer whole with FILL where nothing was written, the slot
    each launch's log-prob record belongs to)"""
    st = dict(st0)
    out = np.full(out_cap, FILL, np.uint32)
    slots = []
    for tok in tokens:
        select_step(st, out, tok, advance)
        slots.append(lp_slot(st["step"], advance))
    return st, out, slots


def lp_slot(step_after, advance):
    return (step_after - advance) % U32


def state_tuple(rec):
    """a STEP_STATE record or a state dict as a plain tuple in field order"""
    return tuple(int(rec[f]) for f in STATE_FIELDS)


# ---- row movement -------------------------------------------------------------------------------------------------------------

def bf16_to_f32(bits):
    """uint16 bf16 bit patterns widened to float32 (exact)"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def embed(table, ids):
    """x[t, :] = table[ids[t], :] as float32"""
    table = np.asarray(table)
    rows = table[np.asarray(ids, dtype=np.int64)]
    return bf16_to_f32(rows) if table.dtype == np.uint16 else rows.astype(np.float32)


def unshard(src):
    """[tp][B][Vs] -> [B][tp * Vs]: out[b, r * Vs + j] = src[r, b, j]"""
    tp, B, Vs = src.shape
    out = np.empty((B, tp * Vs), src.dtype)
    for r in range(tp):
        for b in range(B):
            out[b, r * Vs:(r + 1) * Vs] = src[r, b]
    return out


def gather_last_rows(src, counts, h, dst_slab, fill):
    """src [n_slab, src_slab]: each slab starts with the pack's [sum(counts), h] rows -> [n_slab, dst_slab], slab sl beginning with the
    members' last rows [n_seq, h]; the rest keeps `fill`"""
    n_slab = src.shape[0]
    out = np.full((n_slab, dst_slab), fill, src.dtype)
    last = np.cumsum(counts) - 1
    for sl in range(n_slab):
        for s, r in enumerate(last):
            out[sl, s * h:(s + 1) * h] = src[sl, r * h:(r + 1) * h]
    return out


def reduce_shards(src, reverse=False):
    """the emulated all-reduce: a float32 sum from 0, shard after shard in order (reverse: from the last shard), every operation rounded"""
    s = np.zeros(src.shape[1], np.float32)
    for k in (range(src.shape[0] - 1, -1, -1) if reverse else range(src.shape[0])):
        s = (s + src[k]).astype(np.float32)
    return s


def shard_data(nshards, n, seed=0):
    """float32 [nshards, n] of mixed magnitudes (2^-12 .. 2^12, both signs): with three or more shards the order of the additions shows in
    the low bits of many elements"""
    rng = np.random.default_rng(1000 * nshards + seed)
    mant = rng.uniform(1.0, 2.0, size=(nshards, n))
    exp = rng.integers(-12, 13, size=(nshards, n))
    sign = rng.choice([-1.0, 1.0], size=(nshards, n))
    x = (sign * mant * np.exp2(exp)).astype(np.float32)
    if nshards >= 3:
        # element 0 shows the order by construction: 1 + 2^-24 + 2^-24 is 1 from the left (each half ulp rounds to even) and
        # 1 + 2^-23 from the right
        x[:, 0] = 0.0
        x[0, 0], x[1, 0], x[2, 0] = 1.0, 2.0 ** -24, 2.0 ** -24
    return x


def packed_state(token, pos, len_):
    """what launch_packed_set_states leaves in a member's step state"""
    return state(token=token, pos=pos, len=len_, step=0, eos=-1, done=0, error=0, call0=len_)


def collect(tokens, errors):
    """launch_packed_collect: (token, error) pairs in member order"""
    return np.stack([np.asarray(tokens, np.uint32), np.asarray(errors, np.uint32)], axis=1).reshape(-1)
