"""numpy restatement of guided decoding (include/fastllm_mi355x.h, "guided decoding"): a token-level automaton in CSR form, the
masked row the selection reads -- a COPY of the row with -inf written outside the state's list, so allowed entries keep their bits --
and the walk along a token's edge."""
import numpy as np

NEG_INF = np.float32("-inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def argmax_last(row):
    """ArgMax of the device selection: the LAST maximal index."""
    row = np.asarray(row)
    return int(len(row) - 1 - np.argmax(row[::-1]))


class Automaton:
    """lists[s]: the ascending ids state s allows; nexts[s]: one next state for all of them, or an array as long as the list."""

    def __init__(self, lists, nexts):
        self.lists = [np.asarray(x, dtype=np.uint32) for x in lists]
        self.nexts = [np.full(len(x), n, np.uint32) if np.isscalar(n) else np.asarray(n, dtype=np.uint32) for x, n in zip(self.lists, nexts)]
        self.n_states = len(self.lists)
        self.row_ptr = np.concatenate([[0], np.cumsum([len(x) for x in self.lists])]).astype(np.uint64)
        self.tokens = np.concatenate(self.lists).astype(np.uint32)
        self.next = np.concatenate(self.nexts).astype(np.uint32)

    def csr(self):
        return self.row_ptr, self.tokens, self.next

    def mask(self, row, state):
        row = np.ascontiguousarray(row, dtype=np.float32)
        y = np.full(row.shape, NEG_INF, np.float32)
        idx = self.lists[state]
        y.view(np.uint32)[idx] = row.view(np.uint32)[idx]
        return y

    def walk(self, state, token):
        lst = self.lists[state]
        i = int(np.searchsorted(lst, token))
        return int(self.nexts[state][i]) if i < len(lst) and int(lst[i]) == int(token) else int(state)

    def walk_all(self, state, tokens):
        for t in tokens:
            state = self.walk(state, int(t))
        return state
