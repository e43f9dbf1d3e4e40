// One nucleus-sampling (top-p) step on the device: the next-token logits of every row in, the sampled token out -- no sort and
// no (rows, V) temporaries.  Replaces the sort / softmax / cumsum / shift / scatter_ / masked_fill_ / softmax / multinomial chain
// of virtex/utils/nucleus_sampling.py:78-113 when the decoder is built with draw="device".
//
// Contract (include/virtex_amd.h repeats it).  Per row r: fp32 logits x[0..V), last[r], a caller-supplied uniform u[r] in [0, 1),
// 0 < p < 1.  Every token carries an INTEGER mass w_i = rint(exp(x_i - max x) * 2^40); Z = sum w_i.
//   1. order     descending logit, ties by ascending token index
//   2. nucleus   the token at rank i is kept iff the mass of the ranks before it is <= p Z (rank 0 always; the token that
//                crosses the threshold is kept, nucleus_sampling.py:83-91); kept = their number
//   3. candidates = the kept tokens except last[r] (:101)
//   4. draw      M = mass of the candidates, t = floor(floor(u 2^24) M / 2^24): the first candidate, in rank order, whose
//                inclusive cumulative mass exceeds t
//   5. no candidates (last[r] alone is the nucleus): the reference's softmax over V logits of -1e12 is uniform ->
//                min(floor(u V), V - 1)
//   6. last[r] == eos: eos (:113); kept is written all the same
// p enters as floor(p 2^24) / 2^24 (exact for p >= 0.5).  Integer sums commute: LDS atomics give the same bits on every run,
// and the cut and the draw are exact integer comparisons.
//
// Design: one 1024-thread workgroup per row (four waves per SIMD hide the LDS read and atomic latencies that one wave leaves
// exposed: 49 against 92 us at V = 10000, profiles/nucleus_step.txt), a WEIGHTED RADIX SELECT instead of a sort.  "The first rank whose inclusive
// cumulative mass exceeds a target" is found by descending a 5-digit key, most significant digit first; each round builds a
// 256-bin LDS histogram of (mass u64, count u32) over the elements that match the digits chosen so far, and wave 0 scans
// the bins with shuffles for the bin in which the running mass crosses the target.
//   digit 0      min(255, floor((max - x) * 8)): monotone in x, so a bin is a contiguous range of ranks.  The top byte of the
//                float key alone (sign + 7 exponent bits) sends a whole vocabulary to ~6 bins -- every lane of a wave on the
//                same LDS address; this digit spreads it over the 256 bins first (a departure from a plain 4 x 8-bit descent)
//   digits 1-4   the four bytes of an order-preserving 32-bit key of x, inside the chosen digit-0 bin
// After the last round the survivors share one key, hence one mass: the ordinal of the crossing token among them is a division,
// and its token index a count over indices (256 contiguous chunks, the same bin scan over the per-thread counts).
// The select runs twice: target floor(p Z) over all tokens -> the cut token and `kept`; target t over the candidates.
// The row's keys stay in LDS across all passes while V <= RESIDENT_V (48 KB of keys + 3.2 KB of histogram and state: under
// the 64 KB a block gets without opting in, so two 1024-thread blocks still share a CU); larger rows re-read the logits
// (L2-resident) every pass.
#include "vtx_common.h"

namespace {

typedef unsigned long long u64;
constexpr int NT = 1024, NW = NT / 64;               // threads / waves of a workgroup
constexpr int RESIDENT_V = 12288;
constexpr int MAX_V = 1 << 22;                       // V * 2^40 < 2^63: floor(a M / 2^24) below stays inside 64 bits
constexpr float MASS_ONE = 1099511627776.0f;         // 2^40

// smaller key = larger logit; -0 and +0 are one key; NaN ranks last
__device__ __forceinline__ uint32_t rkey_of(float x) {
    const uint32_t b = __float_as_uint(x + 0.0f);
    return x != x ? 0xffffffffu : (b & 0x80000000u) ? b : (~b & 0x7fffffffu);
}
__device__ __forceinline__ float logit_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k : (~k & 0x7fffffffu)); }
__device__ __forceinline__ u64 mass_of(uint32_t k, float m) {
    const float e = __expf(logit_of(k) - m);
    return e > 0.f ? (u64)rintf(fminf(e, 1.f) * MASS_ONE) : 0ull;          // NaN and underflow: no mass
}
__device__ __forceinline__ uint32_t coarse_of(uint32_t k, float m) { return (uint32_t)fminf((m - logit_of(k)) * 8.f, 255.f); }
// floor(a * M / 2^24), a < 2^24, M < 2^63
__device__ __forceinline__ u64 mulshift24(uint32_t a, u64 M) { return (u64)a * (M >> 24) + (((u64)a * (M & 0xffffffull)) >> 24); }

struct Shared {
    u64 hmass[256];
    unsigned hcnt[256];
    float fred[NW];
    u64 acc, binmass, target;       // written by scan_select
    unsigned cnt, bincnt, digit;
    int idx;
};

// Wave 0, all 64 lanes: the first bin whose inclusive running mass (from `acc`) exceeds the target.  frac24 >= 0: the target is
// floor(frac24 / 2^24 * the histogram's total).  -> s.digit, s.acc / s.cnt (mass / count before that bin), s.binmass / s.bincnt.
__device__ __forceinline__ void scan_select(Shared& s, u64 acc, unsigned cnt, u64 target, int frac24) {
    const int lane = threadIdx.x;
    u64 m[4], ms = 0;
    unsigned c[4], cs = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { m[q] = s.hmass[4 * lane + q]; c[q] = s.hcnt[4 * lane + q]; ms += m[q]; cs += c[q]; }
    u64 mi = ms;
    unsigned ci = cs;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 tm = __shfl(mi, (lane - off) & 63, 64);
        const unsigned tc = __shfl(ci, (lane - off) & 63, 64);
        if (lane >= off) { mi += tm; ci += tc; }
    }
    if (frac24 >= 0) target = mulshift24((uint32_t)frac24, __shfl(mi, 63, 64));
    const u64 hit = __ballot(acc + mi > target);
    const int L = hit ? __builtin_ctzll(hit) : 63;  // no crossing (non-finite logits): the last bin, never out of range
    if (lane == L) {
        u64 a = acc + (mi - ms), bm = m[0];
        unsigned n = cnt + (ci - cs), bc = c[0];
        int q = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (q == k && a + m[k] <= target) { a += m[k]; n += c[k]; q = k + 1; bm = m[k + 1]; bc = c[k + 1]; }
        s.digit = 4 * lane + q; s.acc = a; s.cnt = n; s.binmass = bm; s.bincnt = bc; s.target = target;
    }
}

// which tokens a select ranges over: all of them (the cut), or the candidates (ranks up to the cut token, without `last`)
struct Scope {
    bool candidates;
    uint32_t cut_key;
    int cut_idx;
    long long last;
    __device__ __forceinline__ bool has(uint32_t k, int i) const {
        return !candidates || ((k < cut_key || (k == cut_key && i <= cut_idx)) && (long long)i != last);
    }
};

struct Row {
    const float* x;
    const uint32_t* keys;           // LDS copy of the row's keys, or null: re-read the logits
    int V;
    float m;
    __device__ __forceinline__ uint32_t key(int i) const { return keys ? keys[i] : rkey_of(x[i]); }
};

struct Found { uint32_t key; u64 before, w; unsigned rank_before, ordinal; int idx; };

// the token of `scope` at which the inclusive cumulative mass, in rank order, first exceeds the target
__device__ __forceinline__ Found weighted_select(Shared& s, const Row& row, const Scope& scope, u64 target, int frac24) {
    const int tid = threadIdx.x;
    u64 acc = 0;
    unsigned cnt = 0, coarse = 0, prefix = 0;
    for (int r = 0; r < 5; ++r) {
        if (tid < 256) { s.hmass[tid] = 0; s.hcnt[tid] = 0; }
        __syncthreads();
        const int sh = 32 - 8 * r;                                        // digit r >= 1 = bits [sh, sh + 8) of the key
        uint32_t next = tid < row.V ? row.key(tid) : 0u;
        for (int i = tid; i < row.V; i += NT) {
            const uint32_t k = next;
            if (i + NT < row.V) next = row.key(i + NT);                   // the next key is on its way while this one is binned
            if (!scope.has(k, i) || (r > 0 && (uint32_t)((u64)k >> (sh + 8)) != prefix)) continue;
            const uint32_t c0 = coarse_of(k, row.m);
            if (r > 0 && c0 != coarse) continue;
            const uint32_t d = r == 0 ? c0 : (k >> sh) & 255u;
            atomicAdd(&s.hmass[d], mass_of(k, row.m));
            atomicAdd(&s.hcnt[d], 1u);
        }
        __syncthreads();
        if (tid < 64) scan_select(s, acc, cnt, target, r == 0 ? frac24 : -1);
        __syncthreads();
        acc = s.acc; cnt = s.cnt; target = s.target;
        if (r == 0) coarse = s.digit; else prefix = (prefix << 8) | s.digit;
    }
    Found f;
    f.key = prefix; f.before = acc; f.rank_before = cnt;
    const unsigned n_eq = s.bincnt;
    f.w = n_eq ? s.binmass / n_eq : 0;
    u64 j = f.w && target >= acc ? (target - acc) / f.w : 0;
    if (n_eq && j > n_eq - 1) j = n_eq - 1;
    f.ordinal = (unsigned)j;
    // its token index: the j-th token of the scope with this key, in index order
    const int chunk = (row.V + 255) / 256, lo = tid * chunk, hi = min(lo + chunk, row.V);
    unsigned mine = 0;
    for (int i = lo; i < hi; ++i) { const uint32_t k = row.key(i); mine += k == f.key && scope.has(k, i); }
    __syncthreads();
    if (tid < 256) { s.hmass[tid] = mine; s.hcnt[tid] = mine; }
    if (tid == 0) s.idx = 0;
    __syncthreads();
    if (tid < 64) scan_select(s, 0, 0, j, -1);
    __syncthreads();
    if (tid == (int)s.digit) {
        unsigned left = (unsigned)(j - s.acc);
        for (int i = lo; i < hi; ++i) {
            const uint32_t k = row.key(i);
            if (k == f.key && scope.has(k, i) && left-- == 0) { s.idx = i; break; }
        }
    }
    __syncthreads();
    f.idx = s.idx;
    return f;
}

__global__ __launch_bounds__(NT) void nucleus_step_kernel(const float* __restrict__ logits, long ld, const long long* __restrict__ last,
                                                           const float* __restrict__ u, int V, int eos, int p24, int resident,
                                                           long long* __restrict__ token_out, int* __restrict__ kept_out) {
    __shared__ Shared s;
    HIP_DYNAMIC_SHARED(uint32_t, keys)
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (long)r * ld;
    float m = -INFINITY;
    if ((((uintptr_t)logits | (uintptr_t)(ld * sizeof(float))) & 15) == 0) {          // base AND stride: every row is 16-byte aligned
        for (int i = tid; i < V / 4; i += NT) {
            const float4 v = reinterpret_cast<const float4*>(x)[i];
            m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
            if (resident) { keys[4 * i] = rkey_of(v.x); keys[4 * i + 1] = rkey_of(v.y); keys[4 * i + 2] = rkey_of(v.z); keys[4 * i + 3] = rkey_of(v.w); }
        }
        for (int i = (V & ~3) + tid; i < V; i += NT) { m = fmaxf(m, x[i]); if (resident) keys[i] = rkey_of(x[i]); }
    } else {
        for (int i = tid; i < V; i += NT) { m = fmaxf(m, x[i]); if (resident) keys[i] = rkey_of(x[i]); }
    }
    m = block_max<NW>(m, s.fred);                    // its barriers also publish the keys
    const Row row{x, resident ? keys : nullptr, V, m};
    const long long prev = last[r];

    const Found cut = weighted_select(s, row, Scope{false, 0u, 0, -1}, 0, p24);
    const int kept = (int)(cut.rank_before + cut.ordinal) + 1;
    if (tid == 0) kept_out[r] = kept;
    if (prev == (long long)eos) {
        if (tid == 0) token_out[r] = eos;
        return;
    }
    u64 M = cut.before + (u64)(cut.ordinal + 1) * cut.w;                   // inclusive cumulative mass at the cut token
    if (prev >= 0 && prev < V) {
        const uint32_t k = row.key((int)prev);
        if (k < cut.key || (k == cut.key && prev <= cut.idx)) M -= mass_of(k, m);
    }
    const float uu = fminf(fmaxf(u[r], 0.f), 0.99999994f);
    if (M == 0) {                                   // no candidates: uniform over the vocabulary
        if (tid == 0) token_out[r] = min((int)((double)uu * (double)V), V - 1);
        return;
    }
    const u64 t = mulshift24((uint32_t)(uu * 16777216.f), M);
    const Found pick = weighted_select(s, row, Scope{true, cut.key, cut.idx, prev}, t, -1);
    if (tid == 0) token_out[r] = pick.idx;
}

}  // namespace

extern "C" int vtx_nucleus_step(const float* logits, long ld, const long long* last, const float* u, int rows, int V, int eos, float p,
                                long long* token_out, int* kept_out, void* stream) {
    VTX_CHECK(logits && last && u && token_out && kept_out, VTX_ERR_ARG, "nucleus_step: null pointer");
    VTX_CHECK(rows > 0 && V > 0 && ld >= V, VTX_ERR_ARG, "nucleus_step: bad shape (rows %d, V %d, ld %ld)", rows, V, ld);
    VTX_CHECK(p > 0.f && p < 1.f, VTX_ERR_ARG, "nucleus_step: p = %g is outside (0, 1)", (double)p);
    VTX_CHECK(V <= MAX_V, VTX_ERR_SHAPE, "nucleus_step: V = %d exceeds %d (the 64-bit fixed-point masses would overflow)", V, MAX_V);
    const int resident = V <= RESIDENT_V;
    const int p24 = (int)(p * 16777216.f);
    VTX_KLAUNCH("nucleus_step", 0, 4.0 * rows * V, nucleus_step_kernel, dim3(rows), dim3(NT), resident ? V * sizeof(uint32_t) : 0,
                (hipStream_t)stream, logits, ld, last, u, V, eos, p24, resident, token_out, kept_out);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}
