"""numpy restatement of the adjustment inside a verify step (include/fastllm_mi355x.h, "speculative decode for full requests";
fastllm_amd/csrc/k_verify_adjust.hip), built only from logit_rules_ref.table / count / apply and guide_ref.Automaton.

Row i of a verify step stands for step i of the plain loop, whose input ids[i] (ids[0] the step's token, ids[i] draft[i-1]) is counted
BEFORE the row is adjusted, and whose guide state is the one reached after drafts 0 .. i-1:

    words_i = words counted once for every r <= i (an id that occurs twice: twice; saturating; prompt bit untouched)
    out[i]  = mask(apply(x[i], words_i, bias, rp, fp, pp), state_i)        (rules first, mask last; either may be absent)

The table the launch was given is NOT changed by it; count_rows() is what the step leaves once the caller knows the rows it keeps."""
import numpy as np

import logit_rules_ref as lr


def states(automaton, state0, draft):
    """state_i for the rows of [token, *draft]: state0, then one walk per draft id (an id without an edge leaves the state)."""
    out, s = [int(state0)], int(state0)
    for t in draft:
        s = automaton.walk(s, int(t))
        out.append(s)
    return out


def adjust(x, ids, words=None, bias=None, scalars=(1.0, 0.0, 0.0), automaton=None, row_states=None):
    """x float32 [T, V], ids [T] -> the rows the selection reads, float32 [T, V].  words / bias None: no rules; automaton None: no guide."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    T = x.shape[0]
    out = np.empty_like(x)
    w = None if words is None else np.array(words, dtype=np.uint32)          # a copy: the caller's table stays as it is
    for i in range(T):
        row = x[i]
        if w is not None:
            lr.count(w, int(ids[i]))
            row = lr.apply(row, w, bias, *scalars)
        if automaton is not None:
            row = automaton.mask(row, int(row_states[i]))
        out[i] = row
    return out


def count_rows(words, ids, n_rows):
    """The table after a step that kept rows 0 .. n_rows-1: their inputs counted (a copy)."""
    w = np.array(words, dtype=np.uint32)
    for t in list(ids)[:n_rows]:
        lr.count(w, int(t))
    return w


def accept(rows, draft, select):
    """The ids a step returns: select(i, rows[i]) per row, accepted while they equal the drafts, and the first that does not."""
    got = []
    for i in range(len(draft) + 1):
        got.append(int(select(i, rows[i])))
        if i == len(draft) or got[i] != int(draft[i]):
            break
    return got
