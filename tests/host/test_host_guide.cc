// compile_guide (fastllm_amd/host/guide_compile.hpp) as a stand-alone program, built with AddressSanitizer + UndefinedBehaviorSanitizer
// by tests/test_host_guide.py: a 12-token toy vocabulary with multi-byte tokens, one empty token and one token that is a prefix of
// another, against CSR arrays written out by hand.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "guide_compile.hpp"

using fastllm::GuideTable;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

// id:                          0    1    2     3     4     5   6    7     8      9     10       11
static const char *kVocab[] = {"0", "7", "12", "123", "1a", "", "a", "ab", "abc", "b", "</s>", "90"};
static const size_t kV = 12;
static const uint32_t kEos = 10;

struct Vocab {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets{0};
    Vocab() {
        for (size_t v = 0; v < kV; v++) {
            bytes.insert(bytes.end(), kVocab[v], kVocab[v] + strlen(kVocab[v]));
            offsets.push_back(bytes.size());
        }
        // exactly the promised sizes on the heap: the sanitizer sees a read past either end
        bytes.shrink_to_fit();
        offsets.shrink_to_fit();
    }
};

struct Dfa {
    std::vector<int32_t> t;
    std::vector<uint8_t> acc;
    explicit Dfa(size_t S) : t(S * 256, -1), acc(S, 0) {}
    void edge(int from, const char *bytes, int to) { for (const char *p = bytes; *p; p++) t[(size_t)from * 256 + (uint8_t)*p] = to; }
};

static bool same(const GuideTable &g, std::vector<uint64_t> rp, std::vector<uint32_t> tk, std::vector<uint32_t> nx, uint32_t start) {
    return g.row_ptr == rp && g.tokens == tk && g.next == nx && g.start_state == start;
}

static bool well_formed(const GuideTable &g) {
    if (g.row_ptr.empty() || g.row_ptr[0] != 0 || g.row_ptr.back() != g.tokens.size() || g.tokens.size() != g.next.size()) return false;
    for (size_t s = 0; s + 1 < g.row_ptr.size(); s++) {
        if (g.row_ptr[s + 1] <= g.row_ptr[s]) return false;          // every state has an edge
        for (uint64_t e = g.row_ptr[s]; e < g.row_ptr[s + 1]; e++) {
            if (e > g.row_ptr[s] && g.tokens[e] <= g.tokens[e - 1]) return false;
            if (g.tokens[e] >= kV || g.next[e] >= g.n_states()) return false;
        }
    }
    return g.start_state < g.n_states();
}

int main() {
    const Vocab vocab;
    // case 1: [0-9]+ -- state 0 the start, state 1 (accepting) after one digit or more
    {
        Dfa d(2);
        d.edge(0, "0123456789", 1);
        d.edge(1, "0123456789", 1);
        d.acc[1] = 1;
        const GuideTable g = fastllm::compile_guide(d.t.data(), 2, d.acc.data(), 0, vocab.bytes.data(), vocab.offsets.data(), kV, kEos);
        // the all-digit tokens are 0 "0", 1 "7", 2 "12", 3 "123", 11 "90"; "1a" dies on its second byte, "" is never an edge.
        // state 0: those five -> 1; state 1: the five -> 1, and EOS -> 2; state 2 (terminal): EOS -> 2
        EXPECT(well_formed(g));
        EXPECT(same(g, {0, 5, 11, 12}, {0, 1, 2, 3, 11, 0, 1, 2, 3, 10, 11, 10}, {1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 1, 2}, 0));
        // without an EOS id there is no terminal state, and nothing else changes
        const GuideTable h = fastllm::compile_guide(d.t.data(), 2, d.acc.data(), 0, vocab.bytes.data(), vocab.offsets.data(), kV);
        EXPECT(well_formed(h));
        EXPECT(same(h, {0, 5, 10}, {0, 1, 2, 3, 11, 0, 1, 2, 3, 11}, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, 0));
    }
    // case 2: "abc" with a dead branch -- 0 -a-> 1 -b-> 2 -c-> 3 (accepting); 0 -b-> 4 -a-> 5 -a-> 5 never accepts; 6 -a-> 3 is
    // never reached; and the start is state 0 of 7
    {
        Dfa d(7);
        d.edge(0, "a", 1); d.edge(1, "b", 2); d.edge(2, "c", 3);
        d.edge(0, "b", 4); d.edge(4, "a", 5); d.edge(5, "a", 5);
        d.edge(6, "a", 3);
        d.acc[3] = 1;
        const GuideTable g = fastllm::compile_guide(d.t.data(), 7, d.acc.data(), 0, vocab.bytes.data(), vocab.offsets.data(), kV, kEos);
        // before pruning state 0 has "a" (6) -> 1, "ab" (7) -> 2, "abc" (8) -> 3, "b" (9) -> 4.  States 4 and 5 never accept; state 2
        // needs a "c", which no token spells, so neither it nor state 1 (whose only edge leads to it) reaches state 3 with this
        // vocabulary; state 6 is not reached.  Left: state 0 with "abc" alone -> 1 (old 3), whose EOS leads to 2 (the terminal state)
        EXPECT(well_formed(g));
        EXPECT(same(g, {0, 1, 2, 3}, {8, 10, 10}, {1, 2, 2}, 0));
    }
    // case 2b: the same with a start state that is not 0 and keeps its number's order: states 6 -a-> 3, started at 6
    {
        Dfa d(7);
        d.edge(0, "a", 1);
        d.edge(6, "a", 3); d.edge(6, "b", 6);
        d.acc[3] = 1;
        const GuideTable g = fastllm::compile_guide(d.t.data(), 7, d.acc.data(), 6, vocab.bytes.data(), vocab.offsets.data(), kV, kEos);
        // kept: 3 (as 0), 6 (as 1), terminal (as 2).  state 3: EOS -> 2; state 6: "a" (6) -> 0, "b" (9) -> 1; terminal: EOS
        EXPECT(well_formed(g));
        EXPECT(same(g, {0, 1, 3, 4}, {10, 6, 9, 10}, {2, 0, 1, 2}, 1));
    }
    // case 3: unsatisfiable -- the only accepting state needs a byte no token has
    {
        Dfa d(2);
        d.edge(0, "z", 1);
        d.acc[1] = 1;
        bool refused = false;
        try { (void)fastllm::compile_guide(d.t.data(), 2, d.acc.data(), 0, vocab.bytes.data(), vocab.offsets.data(), kV, kEos); }
        catch (const std::invalid_argument &) { refused = true; }
        EXPECT(refused);
        // ... and a DFA that accepts nothing at all
        Dfa e(1);
        e.edge(0, "a", 0);
        refused = false;
        try { (void)fastllm::compile_guide(e.t.data(), 1, e.acc.data(), 0, vocab.bytes.data(), vocab.offsets.data(), kV, kEos); }
        catch (const std::invalid_argument &) { refused = true; }
        EXPECT(refused);
        // malformed inputs
        refused = false;
        try { (void)fastllm::compile_guide(d.t.data(), 2, d.acc.data(), 2, vocab.bytes.data(), vocab.offsets.data(), kV, kEos); }
        catch (const std::invalid_argument &) { refused = true; }
        EXPECT(refused);
        d.t[5] = 2;
        refused = false;
        try { (void)fastllm::compile_guide(d.t.data(), 2, d.acc.data(), 0, vocab.bytes.data(), vocab.offsets.data(), kV, kEos); }
        catch (const std::invalid_argument &) { refused = true; }
        EXPECT(refused);
    }
    printf(failures ? "host guide driver FAILED %d\n" : "host guide driver done %d\n", failures);
    return failures ? 1 : 0;
}
