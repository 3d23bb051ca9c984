// host_postings_restrict.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h
// files in order; they are not stand-alone headers; this one needs host_keyed.h, host_maxsim_keyed.h and host_maxsim_exact.h).
// Restricted postings (rq_postings_restrict) and the filtered exact multi-vector search over them (rq_exact_search_maxsim_filtered*);
// DESIGN §4.29; kernels: kernels_postings_restrict.h, compiled in inst_postings_restrict.hip.  Nothing of the index, of the source
// postings' arrays or of the filter is written.
#pragma once
#include "kernels_postings_restrict.h"  // (the launch interface only: the kernels are inst_postings_restrict.hip's)

// q = the postings of p's column over the rows f admits: p's segments cut down to their admitted positions in p's order, the
// emptied ones dropped.  q carries p's generation and removal epoch: it is stale exactly when p is.
static rq_status postings_restrict(const rq_postings *p, const rq_filter *f, rq_postings **out) {
    if (!p || !f || !out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    if (f->idx != p->idx) return fail(RQ_ERR_INVALID, "the filter was made for another index");
    RQC(postings_current(p));
    RQC(filter_current(p->idx, f));
    RQC(ensure_device());
    std::unique_ptr<rq_postings> q(new rq_postings());
    q->idx = p->idx, q->generation = p->generation, q->removal_epoch = p->removal_epoch, q->type = p->type, q->column = p->column;
    q->starts.assign(1, 0);
    const uint32_t n = (uint32_t)p->starts.back(), nv = (uint32_t)p->values.size();  // (a position is a u32, so is a count of them)
    if (n == 0 || nv == 0) {
        RQC(q->pos.alloc(0));
        *out = q.release();
        return RQ_OK;
    }
    RQC(postings_device_copy(p));  // the segments' starts and values in device memory (kept on p)
    const uint32_t pc = restrict_chunks(n), sc = restrict_chunks(nv);
    DevBuf<unsigned long long> admit, keep, values_out;
    DevBuf<uint32_t> chunk, rank64, taken, seg_chunk, seg_lo, starts_out, totals;
    RQC(admit.alloc((size_t)pc * RQ_PR_WORDS));
    RQC(rank64.alloc((size_t)pc * RQ_PR_WORDS));
    RQC(chunk.alloc(pc));
    RQC(taken.alloc(n));
    RQC(keep.alloc((size_t)sc * RQ_PR_WORDS));
    RQC(seg_chunk.alloc(sc));
    RQC(seg_lo.alloc(nv));
    RQC(starts_out.alloc((size_t)nv + 1));
    RQC(values_out.alloc(nv));
    RQC(totals.alloc(2));
    PostRestrictArgs a{};
    a.post = p->pos.p, a.allow = f->pos_bits.p, a.starts = p->d_starts.p, a.values = reinterpret_cast<const unsigned long long *>(p->d_values.p);
    a.n = n, a.nv = nv;
    a.admit = admit.p, a.chunk = chunk.p, a.rank64 = rank64.p, a.pos_out = taken.p;
    a.keep = keep.p, a.seg_chunk = seg_chunk.p, a.seg_lo = seg_lo.p, a.starts_out = starts_out.p, a.values_out = values_out.p;
    a.totals = totals.p;
    launch_restrict_admit(a, nullptr);
    launch_restrict_scan(chunk.p, pc, totals.p, nullptr);
    launch_restrict_take(a, nullptr);
    launch_restrict_segments(a, nullptr);
    launch_restrict_scan(seg_chunk.p, sc, totals.p + 1, nullptr);
    launch_restrict_segments_take(a, nullptr);
    uint32_t h_totals[2] = {0, 0};  // the one wait: admitted postings and kept segments size q's arrays
    HIPC(hipMemcpy(h_totals, totals.p, 8, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    const uint32_t rows = h_totals[0], kept = h_totals[1];
    if (rows > n || kept > nv || kept > rows) return fail(RQ_ERR_HIP, "restricted postings: the device passes disagree on their totals");
    if (rows == n) {
        q->pos.take(taken);  // (everything admitted: the scattered copy is the array)
    } else {
        RQC(q->pos.alloc(rows));
        if (rows) HIPC(hipMemcpy(q->pos.p, taken.p, (size_t)rows * 4, hipMemcpyDeviceToDevice));
    }
    std::vector<uint32_t> h_starts((size_t)kept + 1, 0);
    q->values.resize(kept);
    if (kept) {
        HIPC(hipMemcpy(h_starts.data(), starts_out.p, ((size_t)kept + 1) * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(q->values.data(), values_out.p, (size_t)kept * 8, hipMemcpyDeviceToHost));
    }
    q->starts.assign(h_starts.begin(), h_starts.end());
    HIPC(hipStreamSynchronize(nullptr));
    HIPC(hipGetLastError());
    *out = q.release();
    return RQ_OK;
}

// rq_exact_search_maxsim* over restrict(postings, filter): the restricted object is made for the call and freed after it; the
// search itself is the unfiltered entry's, launch for launch.  A null filter is the unfiltered entry.
static rq_status maxsim_exact_filtered(const rq_index *idx, MaxsimExactIO io, const rq_filter *filter, uint32_t nq, const rq_maxsim_params_t *mp,
                                       bool device) {
    std::unique_ptr<rq_postings> made;
    if (filter) {
        RQC(maxsim_exact_checks(idx, io, nq, mp));  // the unfiltered entry's refusals first, in its order
        rq_postings *q = nullptr;
        RQC(postings_restrict(io.post, filter, &q));
        made.reset(q);
        io.post = q;
    }
    return device ? maxsim_exact_device(idx, io, nq, mp) : maxsim_exact_host(idx, io, nq, mp);
}
