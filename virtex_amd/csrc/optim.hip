// Fused optimizer tail of the training step over FLAT fp32 buffers (HBM-bound; 2 launches):
//   total_norm = ||grad_scale * g||_2 ;  clip = min(1, max_norm / (total_norm + 1e-6))
//   g' = clip * grad_scale * g + wd[seg] * p ;  m = momentum * m + g' ;  p -= lr[seg]*lr_mult * m
//   every k-th step (do_lookahead): slow += alpha * (p - slow) ; p = slow
//
// Replaces, with identical arithmetic, the reference's
//   torch.nn.utils.clip_grad_norm_ (scripts/pretrain_virtex.py:158),
//   optim.SGD(momentum) over 202 one-tensor param groups (virtex/factories.py:529-545),
//   Lookahead.step (virtex/optim/lookahead.py:82-102)
// i.e. ~1000 tiny foreach launches -> 1 reduction + 1 update kernel.  Parameters, gradients,
// momentum and slow weights share ONE layout (the data-parallel bucket order), described by a
// table of chunks that never straddle a parameter: (offset, length <= 4096, segment id).
// The reference's other optimizer, optim.AdamW (virtex/factories.py:503-545 with OPTIM.OPTIMIZER_NAME "adamw"), is the second
// update kernel below: the same table and reduction, two moment buffers, decoupled decay, bias corrections from the step count.
#include "vtx_common.h"

namespace {

constexpr int CHUNK = 4096;

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ x, long n,
                                                            float* __restrict__ partials) {
    __shared__ float red[4];
    float s = 0.f;
    const long nv = n / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    if (blockIdx.x == 0)
        for (long i = nv * 4 + threadIdx.x; i < n; i += 256) s += x[i] * x[i];
    s = block_sum<4>(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
__global__ __launch_bounds__(1024) void sumsq_final_kernel(const float* __restrict__ partials, int np,
                                                           float* __restrict__ out) {
    __shared__ float red[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < np; i += 1024) s += partials[i];
    s = block_sum<16>(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

__global__ __launch_bounds__(256) void sgd_lookahead_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ slow,
    const long long* __restrict__ chunk_off, const int* __restrict__ chunk_len, const int* __restrict__ chunk_seg,
    const float* __restrict__ seg_lr, const float* __restrict__ seg_wd, float lr_mult, float momentum,
    float grad_scale, const float* __restrict__ sumsq, float max_norm, int do_lookahead, float alpha,
    const float* __restrict__ sched) {
    // sched (optional, device memory): {LR multiplier, Lookahead-sync flag} of THIS step, computed on the device -- a
    // captured hipGraph of the step freezes the by-value arguments (vtx_sgd_lookahead_step_dev)
    if (sched) { lr_mult = sched[0]; do_lookahead = sched[1] != 0.f; }
    const int c = blockIdx.x;
    const long off = chunk_off[c];
    const int len = chunk_len[c], seg = chunk_seg[c];
    const float lr = seg_lr[seg] * lr_mult, wd = seg_wd[seg];
    float gs = grad_scale;
    if (max_norm > 0.f) {
        const float total = sqrtf(sumsq[0]) * grad_scale;
        const float coef = max_norm / (total + 1e-6f);
        gs *= coef < 1.f ? coef : 1.f;
    }
    auto update = [&](float& pv, float gv, float& mv, float& sv) {          // one element; sv is touched on Lookahead steps only
        gv = gv * gs + wd * pv;
        mv = momentum * mv + gv;
        pv -= lr * mv;
        if (do_lookahead) { sv = sv + alpha * (pv - sv); pv = sv; }
    };
    if (((off | len) & 3) == 0) {
        // 16-byte accesses (every chunk of the model qualifies: parameter sizes are multiples of 4): a quarter of the memory
        // instructions of the scalar loop below, same arithmetic per element
        float4* p4 = reinterpret_cast<float4*>(p + off); const float4* g4 = reinterpret_cast<const float4*>(g + off);
        float4* m4 = reinterpret_cast<float4*>(m + off); float4* s4 = reinterpret_cast<float4*>(slow + off);
        for (int i = threadIdx.x; i < len / 4; i += 256) {
            float4 pv = p4[i], mv = m4[i];
            const float4 gv = g4[i];
            float4 sv = do_lookahead ? s4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            update(pv.x, gv.x, mv.x, sv.x); update(pv.y, gv.y, mv.y, sv.y); update(pv.z, gv.z, mv.z, sv.z); update(pv.w, gv.w, mv.w, sv.w);
            m4[i] = mv;
            if (do_lookahead) s4[i] = sv;
            p4[i] = pv;
        }
        return;
    }
    for (int i = threadIdx.x; i < len; i += 256) {
        const long k = off + i;
        float pv = p[k], mv = m[k], sv = do_lookahead ? slow[k] : 0.f;
        update(pv, g[k], mv, sv);
        m[k] = mv;
        if (do_lookahead) slow[k] = sv;
        p[k] = pv;
    }
}

// AdamW in the same chunked layout (torch.optim.AdamW, amsgrad = False, behind clip_grad_norm_, then Lookahead):
//   g' = clip * grad_scale * g ;  p *= 1 - lr*wd ;  m += (g' - m)(1 - b1) ;  v = b2 v + (1 - b2) g'g'
//   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// The betas arrive as their complements cb = 1 - beta: fp32 holds 0.001 to 6e-8 relative but 0.999 only to 1.3e-8
// ABSOLUTE, which is 1.3e-5 relative in log(beta) and so in 1 - beta^t at small t -- a hundred fp32 roundings of step size.
// The bias corrections are computed here, from the step count t, by one thread per workgroup in fp64 as
// -expm1(t log1p(-cb)) and handed round through LDS: the by-value form and the device-schedule form (t = sched[2]) run the
// same arithmetic, and a recording or a captured graph holds no correction that could go stale.
__global__ __launch_bounds__(256) void adamw_lookahead_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, float* __restrict__ slow,
    const long long* __restrict__ chunk_off, const int* __restrict__ chunk_len, const int* __restrict__ chunk_seg,
    const float* __restrict__ seg_lr, const float* __restrict__ seg_wd, float lr_mult, float cb1, float cb2, float eps, int t,
    float grad_scale, const float* __restrict__ sumsq, float max_norm, int do_lookahead, float alpha,
    const float* __restrict__ sched) {
    __shared__ float corr[2];                                               // {1 - b1^t, sqrt(1 - b2^t)}
    if (sched) { lr_mult = sched[0]; do_lookahead = sched[1] != 0.f; t = (int)sched[2]; }
    if (!slow) do_lookahead = 0;                                            // an optimizer without Lookahead owns no slow buffer
    if (threadIdx.x == 0) {
        corr[0] = (float)-expm1((double)t * log1p(-(double)cb1));
        corr[1] = (float)sqrt(-expm1((double)t * log1p(-(double)cb2)));
    }
    __syncthreads();
    const int c = blockIdx.x;
    const long off = chunk_off[c];
    const int len = chunk_len[c], seg = chunk_seg[c];
    const float lr = seg_lr[seg] * lr_mult;
    const float decay = 1.f - lr * seg_wd[seg], step_size = lr / corr[0], sbc2 = corr[1], b2 = 1.f - cb2;
    float gs = grad_scale;
    if (max_norm > 0.f) {
        const float total = sqrtf(sumsq[0]) * grad_scale;
        const float coef = max_norm / (total + 1e-6f);
        gs *= coef < 1.f ? coef : 1.f;
    }
    auto moments = [&](float& pv, float gv, float& mv, float& vv) {         // g = m = v = 0: 0 / (0 + eps) = 0, the decay alone acts
        gv *= gs;
        pv *= decay;
        mv += (gv - mv) * cb1;
        vv = b2 * vv + cb2 * gv * gv;
        pv -= step_size * (mv / (sqrtf(vv) / sbc2 + eps));
    };
    auto lookahead = [&](float& pv, float& sv) { sv = sv + alpha * (pv - sv); pv = sv; };
    if (((off | len) & 3) == 0) {
        float4* p4 = reinterpret_cast<float4*>(p + off); const float4* g4 = reinterpret_cast<const float4*>(g + off);
        float4* m4 = reinterpret_cast<float4*>(m + off); float4* v4 = reinterpret_cast<float4*>(v + off);
        float4* s4 = slow ? reinterpret_cast<float4*>(slow + off) : nullptr;
        for (int i = threadIdx.x; i < len / 4; i += 256) {
            float4 pv = p4[i], mv = m4[i], vv = v4[i];
            const float4 gv = g4[i];
            moments(pv.x, gv.x, mv.x, vv.x); moments(pv.y, gv.y, mv.y, vv.y); moments(pv.z, gv.z, mv.z, vv.z); moments(pv.w, gv.w, mv.w, vv.w);
            m4[i] = mv;
            v4[i] = vv;
            if (do_lookahead) {                                             // every k-th step only: the ordinary step moves 7 words
                float4 sv = s4[i];
                lookahead(pv.x, sv.x); lookahead(pv.y, sv.y); lookahead(pv.z, sv.z); lookahead(pv.w, sv.w);
                s4[i] = sv;
            }
            p4[i] = pv;
        }
        return;
    }
    for (int i = threadIdx.x; i < len; i += 256) {                          // a tensor of odd length misaligns every chunk behind it
        const long k = off + i;
        float pv = p[k], mv = m[k], vv = v[k];
        moments(pv, g[k], mv, vv);
        m[k] = mv;
        v[k] = vv;
        if (do_lookahead) { float sv = slow[k]; lookahead(pv, sv); slow[k] = sv; }
        p[k] = pv;
    }
}

}  // namespace

extern "C" int vtx_optim_chunk_elems(void) { return CHUNK; }

// partials: >= 1024 floats of scratch; out[0] = sum of squares
extern "C" int vtx_sumsq(const float* x, long n, float* partials, float* out, void* stream) {
    VTX_CHECK(x && partials && out && n >= 0, VTX_ERR_ARG, "sumsq: bad args");
    VTX_CHECK(((uintptr_t)x & 15) == 0, VTX_ERR_SHAPE, "sumsq: x must be 16-byte aligned");
    long nb = (n / 4 + 255) / 256;
    if (nb > 1024) nb = 1024;
    if (nb < 1) nb = 1;
    VTX_KLAUNCH("optimizer_sumsq", 0, 4.0 * n, sumsq_partial_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, x, n, partials);
    VTX_KLAUNCH("optimizer_sumsq_final", 0, 4.0 * nb, sumsq_final_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, partials, (int)nb, out);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}

static int sgd_lookahead_launch(float* p, const float* g, float* m, float* slow,
                               const long long* chunk_off, const int* chunk_len, const int* chunk_seg,
                               int nchunks, long n_elems, const float* seg_lr, const float* seg_wd, float lr_mult,
                               float momentum, float grad_scale, const float* sumsq, float max_norm,
                               int do_lookahead, float alpha, const float* sched, void* stream) {
    VTX_CHECK(p && g && m && slow && chunk_off && chunk_len && chunk_seg && seg_lr && seg_wd, VTX_ERR_ARG,
              "sgd_lookahead_step: null pointer");
    VTX_CHECK(max_norm <= 0.f || sumsq, VTX_ERR_ARG, "sgd_lookahead_step: clipping needs the sum of squares");
    if (nchunks <= 0) return VTX_OK;
    // algorithmic bytes: the REAL element count (chunks are padded to CHUNK only in the table, never in memory) x (g read, p and m
    // read + written = 5 words; the Lookahead synchronisation adds slow read + written).  With the schedule on the device the
    // host does not know the phase: the 4-of-5 ordinary steps' 5 words are counted (a lower bound, so a fraction above 1 cannot
    // come from the accounting -- round 5 counted CHUNK x nchunks x 7 and reported 1.14 of the HBM peak)
    const double prof_elems = n_elems > 0 ? (double)n_elems : (double)CHUNK * nchunks;
    VTX_KLAUNCH("optimizer_step", 0, 4.0 * prof_elems * ((do_lookahead && !sched) ? 7 : 5), sgd_lookahead_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, p, g, m, slow, chunk_off,
                       chunk_len, chunk_seg, seg_lr, seg_wd, lr_mult, momentum, grad_scale, sumsq, max_norm,
                       do_lookahead, alpha, sched);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}

extern "C" int vtx_sgd_lookahead_step(float* p, const float* g, float* m, float* slow,
                                      const long long* chunk_off, const int* chunk_len, const int* chunk_seg,
                                      int nchunks, long n_elems, const float* seg_lr, const float* seg_wd, float lr_mult,
                                      float momentum, float grad_scale, const float* sumsq, float max_norm,
                                      int do_lookahead, float alpha, void* stream) {
    return sgd_lookahead_launch(p, g, m, slow, chunk_off, chunk_len, chunk_seg, nchunks, n_elems, seg_lr, seg_wd, lr_mult, momentum, grad_scale,
                                sumsq, max_norm, do_lookahead, alpha, nullptr, stream);
}

// The same step with the two per-step scalars read from DEVICE memory: sched[0] = LR multiplier, sched[1] = 1.0f when this
// step ends with the Lookahead synchronisation (every k-th), else 0.0f -- what a captured hipGraph of the training step
// needs (virtex_amd/graph.py keeps the step counter, the schedule and this pair on the device).
extern "C" int vtx_sgd_lookahead_step_dev(float* p, const float* g, float* m, float* slow,
                                          const long long* chunk_off, const int* chunk_len, const int* chunk_seg,
                                          int nchunks, long n_elems, const float* seg_lr, const float* seg_wd, const float* sched,
                                          float momentum, float grad_scale, const float* sumsq, float max_norm,
                                          float alpha, void* stream) {
    VTX_CHECK(sched, VTX_ERR_ARG, "sgd_lookahead_step_dev: null schedule pointer");
    return sgd_lookahead_launch(p, g, m, slow, chunk_off, chunk_len, chunk_seg, nchunks, n_elems, seg_lr, seg_wd, 0.f, momentum, grad_scale,
                                sumsq, max_norm, 1, alpha, sched, stream);
}

static int adamw_lookahead_launch(float* p, const float* g, float* m, float* v, float* slow,
                                 const long long* chunk_off, const int* chunk_len, const int* chunk_seg,
                                 int nchunks, long n_elems, const float* seg_lr, const float* seg_wd, float lr_mult,
                                 float one_minus_beta1, float one_minus_beta2, float eps, int t, float grad_scale,
                                 const float* sumsq, float max_norm, int do_lookahead, float alpha, const float* sched,
                                 void* stream) {
    VTX_CHECK(p && g && m && v && chunk_off && chunk_len && chunk_seg && seg_lr && seg_wd, VTX_ERR_ARG,
              "adamw_lookahead_step: null pointer");
    VTX_CHECK(slow || sched || !do_lookahead, VTX_ERR_ARG, "adamw_lookahead_step: a Lookahead step needs the slow weights");
    VTX_CHECK(max_norm <= 0.f || sumsq, VTX_ERR_ARG, "adamw_lookahead_step: clipping needs the sum of squares");
    VTX_CHECK(one_minus_beta1 > 0.f && one_minus_beta1 <= 1.f && one_minus_beta2 > 0.f && one_minus_beta2 <= 1.f, VTX_ERR_ARG,
              "adamw_lookahead_step: betas must lie in [0, 1) (got 1 - beta = %g, %g)", one_minus_beta1, one_minus_beta2);
    VTX_CHECK(eps > 0.f, VTX_ERR_ARG, "adamw_lookahead_step: eps must be positive (got %g)", eps);
    VTX_CHECK(sched || t >= 1, VTX_ERR_ARG, "adamw_lookahead_step: t counts the steps including this one, >= 1 (got %d)", t);
    if (nchunks <= 0) return VTX_OK;
    // algorithmic bytes, on the REAL element count as above: g read, p, m and v read + written = 7 words; a host-scheduled
    // Lookahead step adds slow read + written.  The device-schedule form counts 7 for the reason given at the SGD launch.
    const double prof_elems = n_elems > 0 ? (double)n_elems : (double)CHUNK * nchunks;
    VTX_KLAUNCH("optimizer_step", 0, 4.0 * prof_elems * ((do_lookahead && !sched) ? 9 : 7), adamw_lookahead_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, slow,
                       chunk_off, chunk_len, chunk_seg, seg_lr, seg_wd, lr_mult, one_minus_beta1, one_minus_beta2, eps, t,
                       grad_scale, sumsq, max_norm, do_lookahead, alpha, sched);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}

extern "C" int vtx_adamw_lookahead_step(float* p, const float* g, float* m, float* v, float* slow,
                                        const long long* chunk_off, const int* chunk_len, const int* chunk_seg,
                                        int nchunks, long n_elems, const float* seg_lr, const float* seg_wd, float lr_mult,
                                        float one_minus_beta1, float one_minus_beta2, float eps, int t, float grad_scale,
                                        const float* sumsq, float max_norm, int do_lookahead, float alpha, void* stream) {
    return adamw_lookahead_launch(p, g, m, v, slow, chunk_off, chunk_len, chunk_seg, nchunks, n_elems, seg_lr, seg_wd, lr_mult,
                                  one_minus_beta1, one_minus_beta2, eps, t, grad_scale, sumsq, max_norm, do_lookahead, alpha,
                                  nullptr, stream);
}

// The same step with every per-step quantity in DEVICE memory: sched = {LR multiplier, Lookahead flag, step count t}.  The
// count travels in the array the SGD form already reads, not as "device step word + by-value offset": t counts AdamW steps
// and the step word counts the LR schedule (start_step moves one, a loaded checkpoint moves both independently), so an
// offset would be a per-run quantity frozen into the recording.  fp32 holds t exactly up to 2^24 steps.
extern "C" int vtx_adamw_lookahead_step_dev(float* p, const float* g, float* m, float* v, float* slow,
                                            const long long* chunk_off, const int* chunk_len, const int* chunk_seg,
                                            int nchunks, long n_elems, const float* seg_lr, const float* seg_wd,
                                            const float* sched, float one_minus_beta1, float one_minus_beta2, float eps,
                                            float grad_scale, const float* sumsq, float max_norm, float alpha, void* stream) {
    VTX_CHECK(sched, VTX_ERR_ARG, "adamw_lookahead_step_dev: null schedule pointer");
    return adamw_lookahead_launch(p, g, m, v, slow, chunk_off, chunk_len, chunk_seg, nchunks, n_elems, seg_lr, seg_wd, 0.f,
                                  one_minus_beta1, one_minus_beta2, eps, 0, grad_scale, sumsq, max_norm, 1, alpha, sched, stream);
}
