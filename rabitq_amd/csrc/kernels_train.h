// kernels_train.h -- the kernels of the centroid trainer (include/rabitq_hip.h, "centroid training": rq_train_centroids*).
// The contract is DESIGN.md section 4.16 and has a CPU model, tests/train_model.py; every result here is compared with it bit
// for bit, so nothing in this file adds floats in an order that depends on timing: no float atomics, no trees.
//   train_gather_kernel    the sample, gathered as stored (any row type) + the finiteness reduction
//   train_start_kernel     centroid j = transformed sample row floor(j * ns / k)
//   train_changed_kernel   labels that differ from the previous iteration's (and the new labels become the previous ones)
//   train_scatter_kernel   bucket the sample by label under the key label << 32 | position (list_sort_kernel then sorts each
//                          bucket: positions ascending within a label)
//   train_reduce_kernel    the segmented reduction: one wave per (cluster, 64-column slab), strictly left to right
//   train_split_kernel     the empty-cluster splits the host planned from the k counts
#pragma once

// Sample row r of ns drawn from n rows: one per stratum [floor(r n / ns), floor((r + 1) n / ns)), every row in order when ns == n.
// u64 arithmetic: ns <= n < 2^32, so (r + 1) * n does not wrap.
__host__ __device__ __forceinline__ uint64_t rq_train_sample_pos(uint64_t r, uint64_t n, uint64_t ns, uint64_t seed) {
    if (ns == n) return r;
    const uint64_t lo = r * n / ns, hi = (r + 1) * n / ns;
    return lo + rq_mix64(seed * 0x100000001B3ull + r) % (hi - lo);
}

// ns sample rows of d elements of type E (fmt: RQ_ROWS_*; f32 rows: E = float) -> the contiguous ns x d `out`, as stored.  One wave
// per row, four rows per block, grid-stride.  *bad = the lowest sample position holding an element whose W is not finite.
template <typename E>
__global__ __launch_bounds__(256) void train_gather_kernel(const E *__restrict__ rows, uint64_t n, uint32_t d, uint64_t ns, uint64_t seed,
                                                           uint32_t fmt, E *__restrict__ out, uint32_t *__restrict__ bad) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < ns; r += (uint64_t)gridDim.x * 4) {
        const E *src = rows + rq_train_sample_pos(r, n, ns, seed) * d;
        E *dst = out + r * d;
        bool finite = true;
        for (uint32_t c = lane; c < d; c += 64) {
            const E v = src[c];
            dst[c] = v;
            float w;
            if constexpr (sizeof(E) == 4) w = v;
            else if constexpr (sizeof(E) == 2) w = rq_widen_elem(v, fmt);
            else w = rq_widen_byte(v, fmt);
            finite = finite && (__builtin_bit_cast(uint32_t, w) & 0x7F800000u) != 0x7F800000u;
        }
        if (!finite) atomicMin(bad, (uint32_t)r);
    }
}

__global__ __launch_bounds__(256) void train_start_kernel(const float *__restrict__ xs, uint64_t ns, uint32_t k, uint32_t dim,
                                                          float *__restrict__ centroids) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)k * dim) return;
    const uint64_t j = i / dim;
    centroids[i] = xs[(j * ns / k) * dim + (i - j * dim)];
}

__global__ __launch_bounds__(256) void train_changed_kernel(const uint32_t *__restrict__ label, uint32_t *__restrict__ prev, uint64_t ns,
                                                            uint32_t *__restrict__ changed) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool diff = false;
    if (i < ns) {
        const uint32_t l = label[i];
        diff = prev[i] != l;
        prev[i] = l;
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(diff));
    if ((threadIdx.x & 63u) == 0 && cnt) atomicAdd(changed, cnt);
}

__global__ __launch_bounds__(256) void train_scatter_kernel(const uint32_t *__restrict__ label, uint64_t ns, const uint32_t *__restrict__ offsets,
                                                            uint32_t *__restrict__ cursor, unsigned long long *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ns) return;
    const uint32_t c = label[i];
    keys[(uint64_t)offsets[c] + atomicAdd(&cursor[c], 1u)] = ((unsigned long long)c << 32) | (uint32_t)i;
}

// Centroid sums and objective partials.  Work item = (cluster j, slab s of 64 columns); one wave per item, four items per block;
// lane = column, so a member row's slab is one coalesced 256-byte read.  The f32 sum of a column is the chain acc = acc + x over
// the members in ascending sample position (keys sorted within the cluster): the chain is the contract, the loads are not, so
// RQ_TRAIN_AHEAD members are fetched before their adds.  The member list is wave-uniform.  Slab 0 also sums the members' f32
// distances left to right in f64 (every lane the same value; lane 0 stores it).  An empty cluster keeps its centroid; its partial is 0.
#define RQ_TRAIN_AHEAD 8
__global__ __launch_bounds__(256) void train_reduce_kernel(const float *__restrict__ xs, const float *__restrict__ dist,
                                                           const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ offsets,
                                                           uint32_t k, uint32_t dim, float *__restrict__ centroids, double *__restrict__ partial) {
    const uint32_t slabs = dim >> 6, lane = threadIdx.x & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (uint64_t)k * slabs) return;
    const uint32_t j = (uint32_t)(item / slabs), s = (uint32_t)(item - (uint64_t)j * slabs);
    const uint32_t b = offsets[j], cnt = offsets[j + 1] - b;
    const unsigned long long *seg = keys + b;
    const float *col = xs + s * 64 + lane;
    float acc = 0.0f;
    double obj = 0.0;
    uint32_t m = 0;
    for (; m + RQ_TRAIN_AHEAD <= cnt; m += RQ_TRAIN_AHEAD) {
        float v[RQ_TRAIN_AHEAD], dv[RQ_TRAIN_AHEAD];
#pragma unroll
        for (int u = 0; u < RQ_TRAIN_AHEAD; ++u) {
            const uint32_t pos = (uint32_t)seg[m + u];
            v[u] = col[(uint64_t)pos * dim];
            dv[u] = s == 0 ? dist[pos] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < RQ_TRAIN_AHEAD; ++u) acc = acc + v[u], obj = obj + (double)dv[u];
    }
    for (; m < cnt; ++m) {
        const uint32_t pos = (uint32_t)seg[m];
        acc = acc + col[(uint64_t)pos * dim];
        if (s == 0) obj = obj + (double)dist[pos];
    }
    if (cnt) centroids[(uint64_t)j * dim + s * 64 + lane] = acc / (float)cnt;
    if (s == 0 && lane == 0) partial[j] = obj;
}

// ops: n_ops pairs (empty cluster e, donor), applied in order (a donor may be split again, an earlier e may be a later donor):
// cent[e][c] = cent[donor][c] * (c even ? 1 + eps : 1 - eps), then cent[donor][c] *= (c even ? 1 - eps : 1 + eps), eps = 2^-10.
// One block; a thread owns its columns through every op, so the ops need no barrier between them.
__global__ __launch_bounds__(256) void train_split_kernel(const uint32_t *__restrict__ ops, uint32_t n_ops, uint32_t dim, float *__restrict__ centroids) {
    const float up = 1.0f + 0.0009765625f, down = 1.0f - 0.0009765625f;
    for (uint32_t c = threadIdx.x; c < dim; c += 256) {
        const float fe = (c & 1u) ? down : up, fd = (c & 1u) ? up : down;
        for (uint32_t o = 0; o < n_ops; ++o) {
            float *pe = centroids + (uint64_t)ops[2 * o] * dim + c, *pd = centroids + (uint64_t)ops[2 * o + 1] * dim + c;
            const float v = *pd;
            *pe = v * fe;
            *pd = v * fd;
        }
    }
}
