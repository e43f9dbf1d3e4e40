// The classification pretraining head (token_classification / multilabel_classification): global average pool over the
// NHWC feature map and the set-valued ("K-hot") softmax cross-entropy, forward and backward.  All HBM-bound.
//
// Replaces, in the reference, visual_features.view(B, C, -1).permute(0, 2, 1).mean(dim=1) of LinearTextualHead
// (virtex/modules/textual_heads.py:85-91) and the per-instance Python loop of ClassificationModel.forward
// (virtex/models/classification.py:75-96: log_softmax, labels.unique(), `l not in ignore_indices`, mean of the picked
// log-probabilities) together with their autograd backward.
//
// Global average pool.  A thread owns 8 consecutive channels (one 16-byte load in bf16, two in fp32).  A 256-thread block is
// 32 channel groups x 8 position lanes: lane j sums the positions p = j (mod 8) of one image, four positions requested at a
// time before any of them is used.  The 8 partial sums of a channel meet in LDS ([lane][8 x 32 channels], conflict-free both
// ways) and are added in lane order by the thread that writes the channel: the order of the sum is fixed, so the result is
// bit-reproducible.  Grid = ceil(C / 256) x B: for B = 256, 7 x 7 x 2048 that is 2 048 blocks with 6-7 independent loads per
// thread, where a thread per channel group walking the 49 rows alone would sit on one memory latency after the other.
// The backward is a broadcast: the same thread layout, dy / HW converted once and stored HW / 8 times with 16-byte stores.
//
// K-hot cross-entropy.  One 256-thread workgroup per row.  The row's labels are staged in LDS as int32 (256 at a time), with -1
// for everything that does not count: an ignored index, and -- a deviation -- a label outside [0, V), which the reference
// would answer with an index error and this kernel drops.  The label SET is a bitmap of ceil(V / 32) words in LDS, built without
// atomics: thread t owns the words t, t + 256, ... and ORs in the bits of the staged labels that fall into its words
// (V = 10 000, L = 30: 2 words x 30 compares per thread); duplicates cost nothing and K = |set| is the block sum of the
// popcounts.  Then ONE sweep over the row: every thread keeps an online (max, sum of exp) pair and, in the same sweep, the sum
// of the logits whose bit is set -- 8 columns per step (two float4 loads, one byte of the bitmap) where the row is 16-byte
// aligned, single columns for the tail and for unaligned rows; V needs no divisibility and no column >= V is ever read.  The
// pairs are merged across the wave with shuffles and across the 4 waves through LDS.  A row with an empty set gives NaN by the
// natural 0 / 0, as the reference's mean of an empty selection does.  The backward rebuilds the bitmap with the same device
// function, makes one sweep and zero-fills the columns [V, ldd) so that the gradient GEMMs can run on a padded class dimension.
#include "vtx_common.h"

namespace {

constexpr int GAP_CH = 8;          // channels per thread
constexpr int GAP_LANES = 8;       // position lanes per block
constexpr int GAP_BATCH = 4;       // positions requested before the first one is used
constexpr int KHOT_MAX_V = 65536;  // 2048 bitmap words = 8 KB of LDS
constexpr int KHOT_WORDS = KHOT_MAX_V / 32;
constexpr int KHOT_STAGE = 256;    // labels staged per round

template <class T>
__global__ __launch_bounds__(256) void gap_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int HW, int C) {
    constexpr int VEC = Elem<T>::VEC, NV = GAP_CH / VEC;
    __shared__ float part[GAP_LANES][256];
    const int cg = threadIdx.x & 31, j = threadIdx.x >> 5;
    const int b = blockIdx.y;
    const int c0 = blockIdx.x * 256 + cg * GAP_CH;
    float acc[GAP_CH];
#pragma unroll
    for (int i = 0; i < GAP_CH; ++i) acc[i] = 0.f;
    if (c0 < C) {      // C % 8 == 0: the whole group exists
        const T* base = x + (long)b * HW * C + c0;
        for (int p = j; p < HW; p += GAP_LANES * GAP_BATCH) {
            uint4 raw[GAP_BATCH][NV];
#pragma unroll
            for (int u = 0; u < GAP_BATCH; ++u) {
                const int pp = min(p + u * GAP_LANES, HW - 1);      // address clamped, value masked below
#pragma unroll
                for (int k = 0; k < NV; ++k) raw[u][k] = *reinterpret_cast<const uint4*>(base + (long)pp * C + k * VEC);
            }
            vtx_loads_issued();
#pragma unroll
            for (int u = 0; u < GAP_BATCH; ++u) {
                if (p + u * GAP_LANES < HW) {
#pragma unroll
                    for (int k = 0; k < NV; ++k) {
                        float f[VEC];
                        vtx_unpack_raw16<T>(raw[u][k], f);
#pragma unroll
                        for (int i = 0; i < VEC; ++i) acc[k * VEC + i] += f[i];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < GAP_CH; ++i) part[j][i * 32 + cg] = acc[i];
    __syncthreads();
    // thread t finishes the channel whose partials sit in column t: group t & 31, element t >> 5 of the group
    const int c = blockIdx.x * 256 + (threadIdx.x & 31) * GAP_CH + (threadIdx.x >> 5);
    if (c < C) {
        float s = part[0][threadIdx.x];
#pragma unroll
        for (int l = 1; l < GAP_LANES; ++l) s += part[l][threadIdx.x];
        Elem<T>::st(y + (long)b * C + c, s / (float)HW);
    }
}

template <class T>
__global__ __launch_bounds__(256) void gap_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int HW, int C) {
    constexpr int VEC = Elem<T>::VEC, NV = GAP_CH / VEC;
    const int cg = threadIdx.x & 31, j = threadIdx.x >> 5;
    const int b = blockIdx.y;
    const int c0 = blockIdx.x * 256 + cg * GAP_CH;
    if (c0 >= C) return;
    Vec16<T> v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        v[k].load(dy + (long)b * C + c0 + k * VEC);
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[k].v[i] = v[k].v[i] / (float)HW;
    }
    T* base = dx + (long)b * HW * C + c0;
    for (int p = j; p < HW; p += GAP_LANES) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k].store(base + (long)p * C + k * VEC);
    }
}

// ---- K-hot cross-entropy ----------------------------------------------------------------------------------------------
struct IgnoreSet {
    int n;
    int idx[8];
};

// The membership bitmap of row `labels[0..L)` in bits[0..ceil(V/32)) (LDS), visible to the whole block on return; returns
// K = the number of distinct labels that count, in every thread.  lab: KHOT_STAGE ints of LDS, red: 4 floats of LDS.
__device__ __forceinline__ float khot_bitmap(const long long* __restrict__ labels, int L, const IgnoreSet& ign, int V,
                                             int* lab, uint32_t* bits, float* red) {
    const int t = threadIdx.x;
    const int nwords = (V + 31) >> 5;
    for (int w = t; w < nwords; w += 256) bits[w] = 0u;        // the words this thread owns: no barrier needed before the ORs
    for (int l0 = 0; l0 < L; l0 += KHOT_STAGE) {
        if (l0) __syncthreads();                               // the previous round has been read
        if (l0 + t < L) {
            const long long v = labels[l0 + t];
            bool ok = v >= 0 && v < V;
            for (int i = 0; i < ign.n; ++i) ok = ok && v != ign.idx[i];
            lab[t] = ok ? (int)v : -1;
        }
        __syncthreads();
        const int n = min(KHOT_STAGE, L - l0);
        for (int w = t; w < nwords; w += 256) {
            uint32_t m = 0u;
            for (int i = 0; i < n; ++i) {
                const int x = lab[i];                          // LDS broadcast
                m |= ((x >> 5) == w) ? (1u << (x & 31)) : 0u;  // -1 >> 5 == -1: never a word
            }
            bits[w] |= m;
        }
    }
    int cnt = 0;
    for (int w = t; w < nwords; w += 256) cnt += __builtin_popcount(bits[w]);
    return block_sum<4>((float)cnt, red);                      // exact: K <= 65 536; its barriers publish the bitmap
}

// (m, s) <- the pair of the union of two column sets; an empty set is (-inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    const float e1 = (m == mn) ? 1.f : __expf(m - mn), e2 = (m2 == mn) ? 1.f : __expf(m2 - mn);
    s = s * e1 + s2 * e2;
    m = mn;
}

__global__ __launch_bounds__(256) void khot_ce_fwd_kernel(const float* __restrict__ logits, long ld,
                                                          const long long* __restrict__ labels, int L, IgnoreSet ign,
                                                          float* __restrict__ lse, float* __restrict__ kcount,
                                                          float* __restrict__ row_loss, int V) {
    __shared__ uint32_t bits[KHOT_WORDS];
    __shared__ int lab[KHOT_STAGE];
    __shared__ float red[4], red_m[4], red_s[4];
    const int r = blockIdx.x, t = threadIdx.x;
    const float K = khot_bitmap(labels + (long)r * L, L, ign, V, lab, bits, red);
    const float* row = logits + (long)r * ld;
    const int V8 = (((uintptr_t)row & 15) == 0) ? (V & ~7) : 0;
    float m = -INFINITY, s = 0.f, sel = 0.f;
    for (int c = t * 8; c < V8; c += 2048) {
        const float4 a = *reinterpret_cast<const float4*>(row + c), b = *reinterpret_cast<const float4*>(row + c + 4);
        const uint32_t by = bits[c >> 5] >> (c & 31);
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        float mx = v[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) mx = fmaxf(mx, v[i]);
        float e = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            e += __expf(v[i] - mx);
            sel += ((by >> i) & 1u) ? v[i] : 0.f;
        }
        lse_merge(m, s, mx, e);
    }
    for (int c = V8 + t; c < V; c += 256) {
        const float v = row[c];
        sel += ((bits[c >> 5] >> (c & 31)) & 1u) ? v : 0.f;
        lse_merge(m, s, v, 1.f);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        lse_merge(m, s, m2, s2);
    }
    sel = block_sum<4>(sel, red);
    if ((t & 63) == 0) { red_m[t >> 6] = m; red_s[t >> 6] = s; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; ++w) lse_merge(m, s, red_m[w], red_s[w]);
        const float l = m + __logf(s);
        lse[r] = l;
        kcount[r] = K;
        row_loss[r] = l - sel / K;       // K == 0: 0 / 0 = NaN, the mean of an empty selection
    }
}

// single block: loss[0] = sum(row_loss) / R
__global__ __launch_bounds__(1024) void khot_reduce_kernel(const float* __restrict__ row_loss, float* __restrict__ loss, int R) {
    __shared__ float red[16];
    float s = 0.f;
    for (int r = threadIdx.x; r < R; r += 1024) s += row_loss[r];
    s = block_sum<16>(s, red);
    if (threadIdx.x == 0) loss[0] = s / (float)R;
}

// dlogits[r][c] = g/R * (exp(logit - lse) - [c in S_r] / K_r) for c < V, 0 for V <= c < ldd
template <class T>
__global__ __launch_bounds__(256) void khot_ce_bwd_kernel(const float* __restrict__ logits, long ld,
                                                          const long long* __restrict__ labels, int L, IgnoreSet ign,
                                                          const float* __restrict__ lse, const float* __restrict__ kcount,
                                                          const float* __restrict__ grad_out, T* __restrict__ dlogits,
                                                          long ldd, int R, int V) {
    constexpr int VEC = Elem<T>::VEC, NV = 8 / VEC;
    __shared__ uint32_t bits[KHOT_WORDS];
    __shared__ int lab[KHOT_STAGE];
    __shared__ float red[4];
    const int r = blockIdx.x, t = threadIdx.x;
    khot_bitmap(labels + (long)r * L, L, ign, V, lab, bits, red);
    const float g = grad_out[0] / (float)R, l = lse[r], hit = 1.f / kcount[r];
    const float* row = logits + (long)r * ld;
    T* drow = dlogits + (long)r * ldd;
    const int V8 = ((((uintptr_t)row | (uintptr_t)drow) & 15) == 0) ? (V & ~7) : 0;
    for (int c = t * 8; c < V8; c += 2048) {
        const float4 a = *reinterpret_cast<const float4*>(row + c), b = *reinterpret_cast<const float4*>(row + c + 4);
        const uint32_t by = bits[c >> 5] >> (c & 31);
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        Vec16<T> o[NV];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i / VEC].v[i % VEC] = g * (__expf(v[i] - l) - (((by >> i) & 1u) ? hit : 0.f));
#pragma unroll
        for (int k = 0; k < NV; ++k) o[k].store(drow + c + k * VEC);
    }
    for (int c = V8 + t; c < V; c += 256)
        Elem<T>::st(drow + c, g * (__expf(row[c] - l) - (((bits[c >> 5] >> (c & 31)) & 1u) ? hit : 0.f)));
    for (long c = V + t; c < ldd; c += 256) Elem<T>::st(drow + c, 0.f);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static inline int make_ignore(const int* ignore, int n_ignore, IgnoreSet* s, const char* who) {
    VTX_CHECK(n_ignore >= 0 && n_ignore <= 8 && (n_ignore == 0 || ignore), VTX_ERR_ARG, "%s: at most 8 ignored indices (got %d)", who, n_ignore);
    s->n = n_ignore;
    for (int i = 0; i < 8; ++i) s->idx[i] = i < n_ignore ? ignore[i] : -1;
    return VTX_OK;
}

template <class T>
void launch_gap(bool fwd, const void* in, void* out, int B, int HW, int C, hipStream_t st) {
    const dim3 grid(vtx_cdiv(C, 256), B);
    const double bytes = (double)sizeof(T) * B * C * (HW + 1.0);
    if (fwd) VTX_KLAUNCH("gap_fwd", 0, bytes, (gap_fwd_kernel<T>), grid, dim3(256), 0, st, (const T*)in, (T*)out, HW, C);
    else VTX_KLAUNCH("gap_bwd", 0, bytes, (gap_bwd_kernel<T>), grid, dim3(256), 0, st, (const T*)in, (T*)out, HW, C);
}

int gap_entry(bool fwd, int dtype, const void* in, void* out, int B, int HW, int C, void* stream) {
    const char* who = fwd ? "gap_fwd" : "gap_bwd";
    VTX_CHECK(in && out, VTX_ERR_ARG, "%s: null pointer", who);
    VTX_CHECK(B > 0 && HW > 0 && C > 0 && B <= 65535, VTX_ERR_ARG, "%s: bad shape %d x %d x %d", who, B, HW, C);
    VTX_CHECK(C % 8 == 0 && aligned16(in) && aligned16(out), VTX_ERR_SHAPE, "%s: C must be a multiple of 8 (got %d), tensors 16-byte aligned", who, C);
    VTX_CHECK(dtype == VTX_BF16 || dtype == VTX_F32, VTX_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
    if (dtype == VTX_BF16) launch_gap<bf16_t>(fwd, in, out, B, HW, C, (hipStream_t)stream);
    else launch_gap<float>(fwd, in, out, B, HW, C, (hipStream_t)stream);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}

}  // namespace

extern "C" int vtx_gap_fwd(int dtype, const void* x, void* y, int B, int HW, int C, void* stream) {
    return gap_entry(true, dtype, x, y, B, HW, C, stream);
}

extern "C" int vtx_gap_bwd(int dtype, const void* dy, void* dx, int B, int HW, int C, void* stream) {
    return gap_entry(false, dtype, dy, dx, B, HW, C, stream);
}

extern "C" int vtx_khot_ce_fwd(const float* logits, long ld, const long long* labels, int L, const int* ignore, int n_ignore,
                               float* lse, float* kcount, float* row_loss, float* loss, int R, int V, void* stream) {
    VTX_CHECK(logits && labels && lse && kcount && row_loss && loss, VTX_ERR_ARG, "khot_ce_fwd: null pointer");
    VTX_CHECK(R > 0 && V > 0 && L >= 1, VTX_ERR_ARG, "khot_ce_fwd: bad shape R = %d, V = %d, L = %d", R, V, L);
    VTX_CHECK(V <= KHOT_MAX_V && ld >= V, VTX_ERR_SHAPE, "khot_ce_fwd: V = %d must be <= %d and <= ld = %ld", V, KHOT_MAX_V, ld);
    IgnoreSet ign;
    if (int rc = make_ignore(ignore, n_ignore, &ign, "khot_ce_fwd")) return rc;
    hipStream_t st = (hipStream_t)stream;
    VTX_KLAUNCH("khot_ce_fwd", 0, 4.0 * R * V + 8.0 * R * L, khot_ce_fwd_kernel, dim3(R), dim3(256), 0, st, logits, ld, labels, L, ign,
                lse, kcount, row_loss, V);
    VTX_KLAUNCH("khot_ce_reduce", 0, 4.0 * R, khot_reduce_kernel, dim3(1), dim3(1024), 0, st, (const float*)row_loss, loss, R);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}

extern "C" int vtx_khot_ce_bwd(int dtype, const float* logits, long ld, const long long* labels, int L, const int* ignore,
                               int n_ignore, const float* lse, const float* kcount, const float* grad_out, void* dlogits,
                               long ldd, int R, int V, void* stream) {
    VTX_CHECK(logits && labels && lse && kcount && grad_out && dlogits, VTX_ERR_ARG, "khot_ce_bwd: null pointer");
    VTX_CHECK(R > 0 && V > 0 && L >= 1, VTX_ERR_ARG, "khot_ce_bwd: bad shape R = %d, V = %d, L = %d", R, V, L);
    VTX_CHECK(V <= KHOT_MAX_V && ld >= V && ldd >= V, VTX_ERR_SHAPE, "khot_ce_bwd: V = %d must be <= %d, <= ld = %ld and <= ldd = %ld", V,
              KHOT_MAX_V, ld, ldd);
    VTX_CHECK(dtype == VTX_BF16 || dtype == VTX_F32, VTX_ERR_DTYPE, "khot_ce_bwd: bad dtype %d", dtype);
    IgnoreSet ign;
    if (int rc = make_ignore(ignore, n_ignore, &ign, "khot_ce_bwd")) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == VTX_BF16)
        VTX_KLAUNCH("khot_ce_bwd", 0, 4.0 * R * V + 2.0 * R * ldd, (khot_ce_bwd_kernel<bf16_t>), dim3(R), dim3(256), 0, st, logits, ld, labels, L,
                    ign, lse, kcount, grad_out, (bf16_t*)dlogits, ldd, R, V);
    else
        VTX_KLAUNCH("khot_ce_bwd", 0, 4.0 * R * V + 4.0 * R * ldd, (khot_ce_bwd_kernel<float>), dim3(R), dim3(256), 0, st, logits, ld, labels, L,
                    ign, lse, kcount, grad_out, (float*)dlogits, ldd, R, V);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}
