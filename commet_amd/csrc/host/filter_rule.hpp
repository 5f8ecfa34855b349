// filter_rule.hpp — the read filter's rule, stated once (reference: src/filter_reads.cpp:186-205, 265-306): what
// happens to a read given its length and base counts, the Shannon index with the reference's float / double mix, and
// the sequential loop over a file's verdicts (the stop at an empty record or at the -m cap, the counters, the bits).
//
// HIP-free on purpose: host/filter_reads.cpp (the tool) and the library's device filter (read_filter.hpp,
// capi/filter.hpp: commet_readset_filter) include the same header, and libcommet_plan.so exports the two functions at
// the end to the CPU tests (host/plan_capi.cpp).
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

namespace commet_host {

// what the reference's loop does with a read (filter_reads.cpp:186-200), decided from its statistics alone
enum Verdict : uint8_t { KEEP = 0, RM_LENGTH = 1, RM_N = 2, RM_SHANNON = 3, EMPTY = 4 };

// the criteria as the tool's command line sets them: -l, -n (INT_MAX: any), -e
struct FilterRule {
    int min_size = 0;
    int max_N = INT_MAX;
    float min_shannon = 0.0f;
    // else the verdict depends on the length alone
    bool needs_bases() const { return max_N != INT_MAX || min_shannon > 0; }
};

// the memo of the tool stops here, and so does the table the device reads: longer reads get their terms computed one by one
constexpr uint64_t SHANNON_TABLE_MAX_LEN = 1024;

// One term of the index (filter_reads.cpp:277-303): f * log(f) / log(2) with f = (float) count / (float) len, the product
// and the quotient in double.  It depends on (count, len) only; count >= 1.
inline double shannon_term(uint64_t count, uint64_t len)
{
    const float f = (float) count / (float) len;
    return f * log(f) / log(2);
}

// filter_reads.cpp:265-306, same float / double mix:  index (float) += term, over A C G T other, skipping absent classes.
// The double term is remembered per worker for the read lengths that occur.
struct Shannon {
    std::vector<std::vector<double>> memo;   // memo[len][count], NaN = not computed yet
    float operator()(const uint64_t cnt[5], uint64_t len)
    {
        float index = 0;
        for (int i = 0; i < 5; ++i) {
            if (cnt[i] == 0) continue;       // (f == 0 in the reference: a quotient of a positive count is never 0)
            double term;
            if (len <= SHANNON_TABLE_MAX_LEN) {
                if (memo.size() <= len) memo.resize(len + 1);
                std::vector<double> &row = memo[len];
                if (row.empty()) row.assign(len + 1, std::nan(""));
                double &slot = row[cnt[i]];
                if (slot != slot) slot = shannon_term(cnt[i], len);
                term = slot;
            } else {
                term = shannon_term(cnt[i], len);
            }
            index += term;
        }
        return fabs(index);
    }
};

// the order of the tests (filter_reads.cpp:188-199): empty -> length -> N -> Shannon.  cnt: A C G T other.
inline uint8_t classify(const FilterRule &rule, uint64_t len, const uint64_t cnt[5], Shannon &sh)
{
    if (len == 0) return EMPTY;
    if ((int) len < rule.min_size) return RM_LENGTH;
    if ((long) cnt[4] > (long) rule.max_N) return RM_N;
    // the index is |...| >= 0: only a positive threshold can remove a read (the usual -e 0 never computes it)
    if (rule.min_shannon > 0 && sh(cnt, len) < rule.min_shannon) return RM_SHANNON;
    return KEEP;
}

struct FilterCounts {
    uint64_t reads = 0;                      // records of the file
    uint64_t selected = 0, removed_length = 0, removed_n = 0, removed_shannon = 0;   // among the reads before the stop
};

// The sequential loop (filter_reads.cpp:186-205) over the verdicts of one file, read by read: it stops at the first
// empty record or once nb_selected >= max_reads (max_reads < 0: the file's reads), the counters count only the reads
// before the stop, and untag_last_reads clears everything from the look-ahead read on when the cap was reached (a
// vector starts all ones, so behind an empty record the bits stay set).  clear(r): read r of the file loses its bit.
template <class VerdictAt, class Clear>
inline FilterCounts filter_loop(uint64_t n_reads, long max_reads, VerdictAt &&verdict_at, Clear &&clear)
{
    FilterCounts fc;
    fc.reads = n_reads;
    if (max_reads == -1) max_reads = (long) n_reads;
    long nb_selected = 0;
    uint64_t pos = 0;                        // current_read_pos
    for (; pos < n_reads; ++pos) {
        const uint8_t v = verdict_at(pos);
        if (nb_selected >= max_reads || v == EMPTY) break;   // loop condition of filter_reads.cpp:186
        if (v == KEEP) ++nb_selected;
        else {
            clear(pos);
            if (v == RM_LENGTH) ++fc.removed_length;
            else if (v == RM_N) ++fc.removed_n;
            else ++fc.removed_shannon;
        }
    }                                        // (pos: the look-ahead get_next_read, filter_reads.cpp:200)
    if (nb_selected >= max_reads)            // untag_last_reads: everything from the look-ahead read on
        for (uint64_t r = pos; r < n_reads; ++r) clear(r);
    fc.selected = (uint64_t) nb_selected;
    return fc;
}

// ---- what the device filter needs of the rule ----------------------------------------------------------------------

// The Shannon terms of the read lengths len_lo .. len_hi (len_hi <= SHANNON_TABLE_MAX_LEN), row after row: the row of
// length L holds L + 1 doubles, the term of (count, L) at shannon_table_at(len_lo, L, count); count 0 is never read (0).
// The very expression the tool evaluates, so a sum of table entries in the reference's order and types IS the tool's index.
inline uint64_t shannon_table_at(uint64_t len_lo, uint64_t len, uint64_t count)
{
    return (len * (len + 1) - len_lo * (len_lo + 1)) / 2 + count;
}
inline uint64_t shannon_table_size(uint64_t len_lo, uint64_t len_hi)
{
    return len_hi < len_lo ? 0 : shannon_table_at(len_lo, len_hi + 1, 0);
}
inline void fill_shannon_table(uint64_t len_lo, uint64_t len_hi, double *out)
{
    for (uint64_t len = len_lo; len <= len_hi; ++len) {
        double *row = out + shannon_table_at(len_lo, len, 0);
        row[0] = 0;
        for (uint64_t c = 1; c <= len; ++c) row[c] = shannon_term(c, len);
    }
}

// The same loop from per-read verdict BITMAPS over a set (64 reads per word, LSB first; read r of the set at bit r & 63 of
// word r >> 6): keep / removed by length / removed by N — a read in none of them was removed by Shannon.  The file is
// reads [first, first + count) of the set, empty_reads the set's empty records in ascending order (their bits in the
// three bitmaps mean nothing).  Walks 64 reads per step; writes the file's final bits into `out`, a bitmap over the set
// laid out like the inputs (only the file's bits are touched).  max_reads < 0: all.
inline FilterCounts finish_file(const uint64_t *keep, const uint64_t *rm_length, const uint64_t *rm_n, uint64_t first, uint64_t count,
                                const uint64_t *empty_reads, uint64_t n_empty, int64_t max_reads, uint64_t *out)
{
    FilterCounts fc;
    fc.reads = count;
    if (count == 0) return fc;
    const uint64_t end = first + count;
    if (max_reads < 0) max_reads = (int64_t) count;
    // where the loop stops for an empty record: the first one of the file
    const uint64_t *e = std::lower_bound(empty_reads, empty_reads + n_empty, first);
    const uint64_t stop_empty = (e != empty_reads + n_empty && *e < end) ? *e : end;
    auto range_mask = [](uint64_t w, uint64_t a, uint64_t b) -> uint64_t {   // bits of word w that are reads of [a, b)
        const uint64_t lo = w * 64, hi = lo + 64;
        if (b <= lo || a >= hi) return 0;
        uint64_t m = ~0ull;
        if (a > lo) m &= ~0ull << (a - lo);
        if (b < hi) m &= ~0ull >> (hi - b);
        return m;
    };
    // the reads the loop looks at: [first, seen), ending behind the read that makes nb_selected reach the cap, or at stop_empty
    uint64_t seen = first;
    bool capped = max_reads == 0;
    for (uint64_t w = first >> 6; !capped && w * 64 < stop_empty; ++w) {
        uint64_t m = range_mask(w, first, stop_empty);
        const uint64_t k = keep[w] & m;
        const uint64_t room = (uint64_t) max_reads - fc.selected;
        if ((uint64_t) __builtin_popcountll(k) >= room) {          // the cap is reached inside this word: at its room-th kept read
            uint64_t kk = k;
            for (uint64_t i = 1; i < room; ++i) kk &= kk - 1;
            const unsigned last = (unsigned) __builtin_ctzll(kk);
            m &= last == 63 ? ~0ull : ((1ull << (last + 1)) - 1);
            capped = true;
            seen = w * 64 + last + 1;
        } else {
            seen = std::min(stop_empty, w * 64 + 64);
        }
        const uint64_t kept = keep[w] & m, by_len = rm_length[w] & m & ~kept, by_n = rm_n[w] & m & ~kept & ~by_len;
        fc.selected += (uint64_t) __builtin_popcountll(kept);
        fc.removed_length += (uint64_t) __builtin_popcountll(by_len);
        fc.removed_n += (uint64_t) __builtin_popcountll(by_n);
        fc.removed_shannon += (uint64_t) __builtin_popcountll(m & ~kept & ~by_len & ~by_n);
    }
    if (fc.selected >= (uint64_t) max_reads) capped = true;         // (reached with the last read looked at, or max_reads = 0)
    // bits: kept reads among those looked at; behind them nothing when the cap was reached, everything otherwise
    for (uint64_t w = first >> 6; w * 64 < end; ++w) {
        const uint64_t file = range_mask(w, first, end), looked = range_mask(w, first, seen);
        const uint64_t bits = (keep[w] & looked) | (capped ? 0 : file & ~looked);
        out[w] = (out[w] & ~file) | (bits & file);
    }
    return fc;
}

}  // namespace commet_host
