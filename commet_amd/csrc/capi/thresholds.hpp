// capi/thresholds.hpp — what a profile call leaves of its byte arrays, and commet_hits_to_tags
// (a part of the one translation unit capi.hip: included there, in order, after many.hpp and before profile.hpp)
//
// The hit-count bytes of a profile are final on the device at the end of commet_index_and_profile (c->d_hits + at[s]) and at the end
// of a shared pass of commet_index_many_and_profile (c->d_hits + q * stride).  HitsLeave is the one download step behind both: per
// byte array either the bytes themselves, as those two calls hand them back, or — the thresholds calls — the tag vectors of the
// thresholds t_first .. t_first + n_t - 1 and the per-file counts of the matrix, made there by hits_tags_kernel (hits_tags.hpp), so
// that only bits come down.  queue() goes in front of the call's one wait for the stream, finish() behind it.
// No room for the words on the device (file ends, counts and tag words of all arrays of the call in ONE kept buffer, c->d_twords):
// the bytes come down instead and finish() thresholds them in a plain host loop — the same result.
#pragma once

namespace {

struct HitsItem {
    const uint8_t *d_hits = nullptr;            // n bytes on the device, on a 16-byte boundary
    uint64_t n = 0;
    const std::vector<FileSpan> *files = nullptr;   // the array's files: contiguous runs of its reads (tags and counts only)
    uint8_t *bytes = nullptr;                   // leave the bytes here (n of them); or, n_t > 0:
    int t_first = 0, n_t = 0;
    uint8_t *const *tags = nullptr;             // n_t vectors of n / 8 + 1 bytes; the array and any entry may be null
    uint64_t *const *shared = nullptr;          // n_t rows of one count per file; the array and any entry may be null
    uint64_t n_files() const { return files ? files->size() : 0; }
    uint64_t tag_words() const { return n / 64 + 1; }
    bool counts() const { return shared != nullptr && n_files() > 0; }
};

int launch_hits_tags(commet_ctx *c, const uint8_t *d_hits, uint64_t n, int t_first, int n_t, uint64_t *d_tags, const uint64_t *d_file_end, int n_files,
                     unsigned long long *d_shared)
{
    const uint64_t tiles = (n / 64 + 1 + 63) / 64;
    const uint64_t cap = (uint64_t) c->hits_tags_blocks;           // (2048: eight workgroups per CU; option "hits_tags_blocks")
    const uint64_t per_block = (tiles + cap - 1) / cap;
    const uint64_t blocks = (tiles + per_block - 1) / per_block;
    KScope ks(c, "hits_tags_kernel", c->stream);
    COMMET_LAUNCH(hits_tags_kernel, dim3((unsigned) blocks), dim3(256), 0, c->stream, d_hits, n, t_first, n_t, d_tags, n / 64 + 1, d_file_end, n_files,
                  d_shared, per_block);
    HIP_OK(hipGetLastError());
    return 0;
}

struct HitsLeave {
    std::vector<HitsItem> items;
    std::vector<uint64_t> h_ends;               // the file ends of every item, as they go up
    std::vector<std::vector<uint8_t>> h_bytes;  // host path: the bytes of every item that wants tags
    std::vector<std::vector<uint64_t>> h_counts;   // device path: an item's n_t x n_files counts as they come down
    bool on_host = false;

    void bytes_of(const uint8_t *d_hits, uint64_t n, uint8_t *to)
    {
        HitsItem it;
        it.d_hits = d_hits, it.n = n, it.bytes = to;
        items.push_back(it);
    }
    void tags_of(const uint8_t *d_hits, const commet_readset *rs, int t_first, int n_t, uint8_t *const *tags, uint64_t *const *shared)
    {
        HitsItem it;
        it.d_hits = d_hits, it.n = rs->n_reads, it.files = &rs->files, it.t_first = t_first, it.n_t = n_t, it.tags = tags, it.shared = shared;
        items.push_back(it);
    }

    // everything of the call queued on the context's stream: copies of bytes, kernels, copies of words and counts
    int queue(commet_ctx *c)
    {
        uint64_t n_ends = 0, n_cnt = 0, n_words = 0;
        for (const HitsItem &it : items) {
            if (!it.n_t) {
                if (it.bytes && it.n) HIP_OK(hipMemcpyAsync(it.bytes, it.d_hits, it.n, hipMemcpyDeviceToHost, c->stream));
                continue;
            }
            n_ends += it.n_files(), n_cnt += (uint64_t) it.n_t * it.n_files(), n_words += (uint64_t) it.n_t * it.tag_words();
        }
        if (!n_words) return 0;
        const uint64_t total = n_ends + n_cnt + n_words;
        if (grow_kept(c, c->d_twords, c->twords_cap, total, total)) {
            // no room: the bytes come down, finish() makes tags and counts of them
            on_host = true;
            h_bytes.resize(items.size());
            for (size_t i = 0; i < items.size(); ++i) {
                const HitsItem &it = items[i];
                if (!it.n_t || !it.n) continue;
                h_bytes[i].resize(it.n);
                HIP_OK(hipMemcpyAsync(h_bytes[i].data(), it.d_hits, it.n, hipMemcpyDeviceToHost, c->stream));
            }
            return 0;
        }
        h_ends.reserve(n_ends);
        for (const HitsItem &it : items)
            if (it.n_t)
                for (const FileSpan &f : *it.files) h_ends.push_back(f.first + f.count);
        uint64_t *d_ends = c->d_twords, *d_cnt = d_ends + n_ends, *d_words = d_cnt + n_cnt;
        if (n_ends) HIP_OK(hipMemcpyAsync(d_ends, h_ends.data(), n_ends * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        if (n_cnt) HIP_OK(hipMemsetAsync(d_cnt, 0, n_cnt * sizeof(uint64_t), c->stream));
        h_counts.resize(items.size());
        for (size_t i = 0; i < items.size(); ++i) {
            const HitsItem &it = items[i];
            if (!it.n_t) continue;
            const uint64_t nf = it.n_files(), tw = it.tag_words();
            if (launch_hits_tags(c, it.d_hits, it.n, it.t_first, it.n_t, d_words, d_ends, (int) nf, it.counts() ? (unsigned long long *) d_cnt : nullptr))
                return 1;
            for (int ti = 0; ti < it.n_t; ++ti)
                if (it.tags && it.tags[ti])
                    HIP_OK(hipMemcpyAsync(it.tags[ti], d_words + (uint64_t) ti * tw, it.n / 8 + 1, hipMemcpyDeviceToHost, c->stream));
            if (it.counts()) {
                h_counts[i].resize((size_t) it.n_t * nf);
                HIP_OK(hipMemcpyAsync(h_counts[i].data(), d_cnt, (uint64_t) it.n_t * nf * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
            }
            d_ends += nf, d_cnt += (uint64_t) it.n_t * nf, d_words += (uint64_t) it.n_t * tw;
        }
        return 0;
    }

    // behind the wait for the stream: the counts to the caller's rows; on the host path tags and counts from the bytes
    void finish()
    {
        for (size_t i = 0; i < items.size(); ++i) {
            const HitsItem &it = items[i];
            if (!it.n_t) continue;
            const uint64_t nf = it.n_files();
            for (int ti = 0; ti < it.n_t; ++ti) {
                uint64_t *row = it.shared ? it.shared[ti] : nullptr;
                if (!on_host) {
                    if (row && nf) memcpy(row, h_counts[i].data() + (size_t) ti * nf, nf * sizeof(uint64_t));
                    continue;
                }
                uint8_t *bits = it.tags ? it.tags[ti] : nullptr;
                if (bits) memset(bits, 0, it.n / 8 + 1);
                const uint8_t t = (uint8_t) (it.t_first + ti);
                const uint8_t *h = h_bytes[i].data();
                for (uint64_t f = 0; f < nf; ++f) {
                    const FileSpan &fs = (*it.files)[f];
                    uint64_t cnt = 0;
                    for (uint64_t r = fs.first; r < fs.first + fs.count; ++r)
                        if (h[r] >= t) {
                            ++cnt;
                            if (bits) bit_on(bits, r);
                        }
                    if (row) row[f] = cnt;
                }
            }
        }
    }
};

}  // namespace

extern "C" {

int commet_hits_to_tags(commet_ctx *c, const uint8_t *hits, uint64_t n_reads, int n_files, const uint64_t *file_reads, int t_first, int n_t,
                        uint8_t *const *tags_out, uint64_t *shared_out)
{
    if (n_files < 0) return fail("n_files must not be negative (got %d)", n_files);
    if (t_first < 1 || n_t < 1 || t_first + n_t - 1 > 255) return fail("thresholds must lie in 1..255 (got %d .. %d)", t_first, t_first + n_t - 1);
    std::vector<FileSpan> files;
    uint64_t total = 0;
    for (int f = 0; f < n_files; ++f) files.push_back(FileSpan{total, file_reads[f]}), total += file_reads[f];
    if (total != n_reads) return fail("the files hold %llu reads, n_reads is %llu", (unsigned long long) total, (unsigned long long) n_reads);
    HIP_OK(hipSetDevice(c->device));
    std::vector<uint64_t *> rows((size_t) n_t, nullptr);
    for (int ti = 0; ti < n_t && shared_out; ++ti) rows[(size_t) ti] = shared_out + (size_t) ti * n_files;
    HitsLeave leave;
    HitsItem it;
    it.n = n_reads, it.files = &files, it.t_first = t_first, it.n_t = n_t, it.tags = tags_out, it.shared = shared_out ? rows.data() : nullptr;
    const uint64_t n_bytes = std::max<uint64_t>((n_reads + 255) & ~255ull, 256);
    if (grow_kept(c, c->d_hits, c->hits_cap, n_bytes, n_bytes)) {
        // no room for the bytes either: the host loop on the caller's own
        leave.on_host = true;
        leave.h_bytes.emplace_back(hits, hits + n_reads);
        leave.items.push_back(it);
        leave.finish();
        return 0;
    }
    if (n_reads) HIP_OK(hipMemcpyAsync(c->d_hits, hits, n_reads, hipMemcpyHostToDevice, c->stream));
    it.d_hits = c->d_hits;
    leave.items.push_back(it);
    int rc = leave.queue(c);
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail("stream synchronize failed: %s", hipGetErrorString(hipGetLastError()));
    c->kclock.collect();
    if (rc) return rc;
    leave.finish();
    return 0;
}

}  // extern "C"
