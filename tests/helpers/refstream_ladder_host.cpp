// Test harness (tests/test_refstream_ladder.py): the window ladder and the accounting rule of dsac_amd/csrc/refstream.h compiled for the host.
#include "../../dsac_amd/csrc/refstream.h"
#include <cstdint>
#include <vector>

extern "C" {

int rsl_window_min() { return rs::WINDOW_MIN; }
int rsl_window_max() { return rs::WINDOW_MAX; }
int rsl_window_per_hyp() { return rs::WINDOW_PER_HYP; }
int rsl_max_windows() { return rs::MAX_WINDOWS; }
int rsl_window_first(int want) { return rs::window_first(want); }
long long rsl_default_budget(int want) { return rs::default_budget(want); }
int rsl_ladder(int want, long long budget, int* sizes, int cap) { return rs::window_ladder(want, budget, sizes, cap); }

// Checks every budget in [b0, b1] for one wanted count: sizes positive, sum == budget, non-decreasing except for the trimmed last one, doubling up to
// WINDOW_MAX, first == window_first(want) unless trimmed, count == what a cap-limited call reports.  Returns the first failing budget, or 0.
long long rsl_check_range(int want, long long b0, long long b1) {
    std::vector<int> s(4096);
    for (long long b = b0; b <= b1; b++) {
        const int n = rs::window_ladder(want, b, s.data(), (int)s.size());
        if (n < 1 || n > (int)s.size()) return b;
        long long sum = 0;
        for (int k = 0; k < n; k++) {
            if (s[k] < 1 || s[k] > rs::WINDOW_MAX) return b;
            sum += s[k];
            if (k + 1 < n) {  // every window but the last is a full rung
                const int rung = k == 0 ? rs::window_first(want) : (s[k - 1] < rs::WINDOW_MAX ? 2 * s[k - 1] : rs::WINDOW_MAX);
                if (s[k] != rung) return b;
            } else if (k > 0 && s[k] > (s[k - 1] < rs::WINDOW_MAX ? 2 * s[k - 1] : rs::WINDOW_MAX)) return b;
            else if (k == 0 && s[k] > rs::window_first(want)) return b;
        }
        if (sum != b) return b;
        int two[2];
        if (rs::window_ladder(want, b, two, 2) != n) return b;
    }
    return 0;
}

// mt_untemper inverts mt_temper: returns the number of mismatches over n words starting at x0 with stride `step` (and the edge words)
long long rsl_untemper_mismatches(uint32_t x0, uint32_t step, long long n) {
    long long bad = 0;
    uint32_t x = x0;
    for (long long i = 0; i < n; i++, x += step) bad += rs::mt_untemper(rs::mt_temper(x)) != x;
    const uint32_t edge[] = {0u, 1u, 0x80000000u, 0xffffffffu, 0x9d2c5680u, 0xefc60000u};
    for (uint32_t e : edge) bad += rs::mt_untemper(rs::mt_temper(e)) != e;
    return bad;
}
// the state of a generator `skip` outputs in, recovered from its outputs alone: the block that holds position `skip` untempered, against twisting up to it
int rsl_state_from_outputs(uint32_t seed, uint64_t skip) {
    std::vector<uint32_t> mt(rs::MT_N), ref(rs::MT_N);
    rs::mt_seed(mt.data(), seed);
    const uint64_t blocks = (skip + rs::MT_N - 1) / rs::MT_N + 1;  // outputs of blocks 1 .. blocks
    std::vector<uint32_t> out;
    for (uint64_t b = 1; b <= blocks; b++) {
        rs::mt_twist_block(mt.data());
        for (int i = 0; i < rs::MT_N; i++) out.push_back(rs::mt_temper(mt[i]));
        if (b == (skip ? (skip - 1) / rs::MT_N + 1 : 1)) ref = mt;
    }
    const uint64_t blk = skip ? (skip - 1) / rs::MT_N : 0;  // block index (0-based among generated) that holds output skip - 1
    int bad = 0;
    for (int i = 0; i < rs::MT_N; i++) bad += rs::mt_untemper(out[blk * rs::MT_N + i]) != ref[i];
    return bad;
}

// The select step's accounting replayed on the host: a stream wants `want` hypotheses, its attempts are accepted where accept[i] != 0 (i counts the
// stream's attempts from the start of the image), the windows are `sizes`.  Returns the attempts charged; *served = hypotheses served.
long long rsl_charge(int want, const uint8_t* accept, long long n_accept, const int* sizes, int n_windows, int* served) {
    long long pos = 0, charged = 0;
    int need = want;
    for (int k = 0; k < n_windows && need > 0; k++) {
        const int parsed = (int)(pos + sizes[k] <= n_accept ? sizes[k] : n_accept - pos);
        int total = 0, last = -1;
        for (int a = 0; a < parsed; a++) {
            if (!accept[pos + a]) continue;
            total++;
            if (total == need) last = a;
        }
        const int used = rs::window_used(total, need, last, parsed);
        need -= total < need ? total : need;
        charged += used;
        pos += used;
        if (parsed < sizes[k]) break;
    }
    *served = want - need;
    return charged;
}

}  // extern "C"
