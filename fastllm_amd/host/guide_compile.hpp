// guide_compile.hpp -- compile_guide: from what grammar / JSON-schema / regex compilers emit, a byte-level DFA, and a vocabulary to the
// token-level automaton fl_guide_create takes (include/fastllm_mi355x.h, "guided decoding").  Pure host code: no GPU, no library
// call, no tokenizer file -- fastllm_host.hpp includes it, and it stands alone for the sanitizer test (tests/host/test_host_guide.cc).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <utility>
#include <vector>

namespace fastllm {

// The CSR arrays of fl_guide_desc and the state a request starts in.
struct GuideTable {
    std::vector<uint64_t> row_ptr;            // [n_states + 1]
    std::vector<uint32_t> tokens, next;       // [nnz]
    uint32_t start_state = 0;
    size_t n_states() const { return row_ptr.empty() ? 0 : row_ptr.size() - 1; }
};

// dfa: dense [S][256] transition table, -1 = no edge, state `start` is where a string begins; accepting [S] (nonzero: the bytes so far
// are a complete match).  The vocabulary is one byte blob, token v = vocab[offsets[v] .. offsets[v + 1]).  For every state and every
// token with a non-empty byte string (the EOS id aside) the bytes are walked through the DFA: a walk that survives is an edge.  With an
// EOS id every accepting state gets an EOS edge into one extra terminal state whose only edge is EOS to itself.  Then, to a fixed
// point, every state is removed that cannot be reached from the start, from which no accepting state can be reached, or that is left
// without an edge (an accepting state without continuation when there is no EOS id), with every edge into a removed state: every
// remaining state has an edge, as fl_guide_create demands.  The remaining states keep their order; the terminal state is the last.
// std::invalid_argument: a malformed input, or an unsatisfiable grammar -- the start state itself was removed.
inline GuideTable compile_guide(const int32_t *dfa, size_t S, const uint8_t *accepting, uint32_t start, const uint8_t *vocab,
                                const uint64_t *offsets, size_t V, std::optional<uint32_t> eos = std::nullopt) {
    if (!dfa || !accepting || !offsets || S == 0 || V == 0) throw std::invalid_argument("compile_guide: empty DFA or vocabulary");
    if (start >= S) throw std::invalid_argument("compile_guide: the start state is not a state");
    if (S >= 0xffffffffull || V > 0xffffffffull) throw std::invalid_argument("compile_guide: too many states or tokens");
    if (eos && *eos >= V) throw std::invalid_argument("compile_guide: the EOS id is not in the vocabulary");
    for (size_t v = 0; v < V; v++)
        if (offsets[v + 1] < offsets[v]) throw std::invalid_argument("compile_guide: vocabulary offsets decrease");
    if (offsets[V] > offsets[0] && !vocab) throw std::invalid_argument("compile_guide: null vocabulary bytes");
    for (size_t i = 0; i < S * 256; i++)
        if (dfa[i] < -1 || (dfa[i] >= 0 && (size_t)dfa[i] >= S)) throw std::invalid_argument("compile_guide: a DFA edge leaves the table");
    const size_t N = S + (eos ? 1 : 0), T = S;                       // T: the terminal state behind EOS
    using Edge = std::pair<uint32_t, uint32_t>;                      // (token, next), ascending by token
    std::vector<std::vector<Edge>> edges(N);
    for (size_t s = 0; s < S; s++) {
        for (size_t v = 0; v < V; v++) {
            if (eos && v == *eos) {
                if (accepting[s]) edges[s].emplace_back((uint32_t)v, (uint32_t)T);
                continue;
            }
            if (offsets[v + 1] == offsets[v]) continue;              // an empty token moves nothing: never allowed
            int32_t at = (int32_t)s;
            for (uint64_t i = offsets[v]; i < offsets[v + 1] && at >= 0; i++) at = dfa[(size_t)at * 256 + vocab[i]];
            if (at >= 0) edges[s].emplace_back((uint32_t)v, (uint32_t)at);
        }
    }
    if (eos) edges[T].emplace_back(*eos, (uint32_t)T);
    auto is_accepting = [&](size_t s) { return s == T ? eos.has_value() : accepting[s] != 0; };
    std::vector<char> keep(N, 1);
    for (bool changed = true; changed;) {
        changed = false;
        // forward: reachable from the start over kept states
        std::vector<char> fwd(N, 0);
        std::vector<uint32_t> stack;
        if (keep[start]) { fwd[start] = 1; stack.push_back(start); }
        while (!stack.empty()) {
            const uint32_t s = stack.back(); stack.pop_back();
            for (const Edge &e : edges[s]) if (keep[e.second] && !fwd[e.second]) { fwd[e.second] = 1; stack.push_back(e.second); }
        }
        // backward: an accepting state can be reached over kept states
        std::vector<char> live(N, 0);
        for (size_t s = 0; s < N; s++) live[s] = keep[s] && is_accepting(s);
        for (bool grew = true; grew;) {
            grew = false;
            for (size_t s = 0; s < N; s++) {
                if (!keep[s] || live[s]) continue;
                for (const Edge &e : edges[s]) if (live[e.second]) { live[s] = 1; grew = true; break; }
            }
        }
        for (size_t s = 0; s < N; s++) {
            if (!keep[s]) continue;
            if (!fwd[s] || !live[s]) { keep[s] = 0; changed = true; }
        }
        for (size_t s = 0; s < N; s++) {                             // edges into removed states go; a state left with none goes too
            if (!keep[s]) { edges[s].clear(); continue; }
            edges[s].erase(std::remove_if(edges[s].begin(), edges[s].end(), [&](const Edge &e) { return !keep[e.second]; }), edges[s].end());
            if (edges[s].empty()) { keep[s] = 0; changed = true; }
        }
    }
    if (!keep[start]) throw std::invalid_argument("compile_guide: the grammar is unsatisfiable with this vocabulary (the start state was removed)");
    std::vector<uint32_t> renumber(N, 0xffffffffu);
    uint32_t n = 0;
    for (size_t s = 0; s < N; s++) if (keep[s]) renumber[s] = n++;
    GuideTable out;
    out.start_state = renumber[start];
    out.row_ptr.push_back(0);
    for (size_t s = 0; s < N; s++) {
        if (!keep[s]) continue;
        for (const Edge &e : edges[s]) { out.tokens.push_back(e.first); out.next.push_back(renumber[e.second]); }
        out.row_ptr.push_back(out.tokens.size());
    }
    return out;
}

}  // namespace fastllm
