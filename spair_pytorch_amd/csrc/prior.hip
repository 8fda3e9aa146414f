// SPAIR.generate: a scene's latents drawn from the model's own prior -- the generative process the loss already assumes (reference:
// _compute_KL, models.py:169-262, evaluates this prior on the posterior's sample; here its own draw takes that sample's place).
//
// k_prior_presence -- the ancestral sampler of the sequential count prior (models.py:184-257).  Cells in row-major order i = h * Gw + w;
//   with cd the distribution of the total object count c = 0 .. HW, `seen` the objects so far and rem = HW - i:
//       q_c = clamp(c - seen, 0, rem) / rem,  p_z(i) = sum_c cd_c q_c,  z_i = [u_i < p_z(i)],
//       cd <- cd (z_i q + (1 - z_i)(1 - q)) / max(its sum, 1e-6),  seen += z_i,
//   started from cd = normalise((1 - p) p^c).  One wave per sample, WPB samples per workgroup, no atomics, no cross-wave traffic: the
//   output is bit-identical from run to run.  The HW + 1 bins live in REGISTERS in RELATIVE form, bin j = c - seen (the idea of k_count_kl,
//   loss.hip): j = (2 k + half) * 64 + lane in half `half` of register PAIR k (packed fp32 pipe).  In that form q_j = j / rem
//   needs no running count and no clamp below; a present cell multiplies bin 0 by q_0 = 0 and every bin then moves down by one lane
//   (wave-rotate DPP and a select per register); an absent cell multiplies bin `rem` by 1 - 1 = 0.  Only the LAST active pair can hold bins past
//   `rem`: its factor is clamped to 1, and 1 / rem is rounded UP whenever rem * (1 / rem) < 1, so the bin AT `rem` gets exactly 1 and
//   the bins past it stay exactly 0 -- no residue that a run of present cells could grow (the dense regime, p ~ 1).  The pairs that can
//   hold mass, floor(rem / 128) + 1, depend on the step alone: the loop is a sequence of phases, each compiled for its pair count; a
//   dropped pair is never read again.
//   Unlike the KL, the factor of a step depends on that step's own p_z.  Both candidates are formed in the one pass that sums p_z:
//   von = cd q (whose sum IS p_z, the normaliser of a present cell) and voff = cd (1 - q) (summed beside it: the normaliser of an absent
//   one), two independent DPP reductions in flight together; the decision u < p_z is on wave-uniform values (p_z comes out of the
//   reduction in a scalar register, u is made uniform), so every lane takes the same branch; then one select-and-scale pass.
//   p_z is stored clamped to <= 1 (the bins sum to 1 within a few ulp); the decision is the same either way, u < 1.
//   EXACT COUNT (count != NULL): the distribution is one-hot at n = clamp(count[b], 0, HW) and the recursion collapses to integers:
//   need = n - seen, p_z = fl32(need / rem) (correctly rounded division: exactly 1 when need == rem, exactly 0 when need == 0),
//   z = [u < p_z].  It runs in that closed form, not through bins (a renormalised one-hot bin drifts by ulps and u = 1 - 2^-24 would
//   miss a forced cell); a forced cell is also taken whatever u holds, so every sample ends with exactly n present cells.
//   u, z and p_z of a sample are staged in LDS (3 HW floats per wave): no global access inside the sequential loop, coalesced stores
//   after it.  Per-sample results are written by lane 0 with ordinary vector stores.
//
// k_prior_gauss -- one thread per (b, channel, cell) of the NCHW outputs, channels = 4 (z_where) + A (z_what) + 1 (z_depth), cell
//   fastest: every load and store is coalesced.  The raw latent is m + s eps with the priors of CellHyper (cy, cx, height, width, attr,
//   depth); the box and depth then go through box_forward / depth_forward of cell_math.h themselves, called with the raw latent as the
//   mean and eps = 0 (mu + sd * 0 = mu, and the freeze is value-preserving), so the transform is the forward's own code.
//
// gfx950 resource usage: DESIGN.md section 7, row f11.
#include "prior.h"
#include "cell_math.h"

namespace {

typedef float pr_f2 __attribute__((ext_vector_type(2)));

// 1 / x: v_rcp_f32 + one Newton step (<= 1 ulp for normal x)
__device__ __forceinline__ float pr_rcp(float x) {
    const float r = __builtin_amdgcn_rcpf(x);
    return fmaf(fmaf(-x, r, 1.f), r, r);
}
// Wave sum, the result wave-uniform (a scalar register): four DPP adds give every lane its 16-lane row's sum, row_bcast:15 / row_bcast:31
// carry the sums up the rows, lane 63 holds the total.
__device__ __forceinline__ float pr_wave_sum(float v) {
    v = dpp_add_<0xB1>(v);      // quad_perm [1,0,3,2]
    v = dpp_add_<0x4E>(v);      // quad_perm [2,3,0,1]
    v = dpp_add_<0x141>(v);     // row_half_mirror
    v = dpp_add_<0x140>(v);     // row_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, false));      // row_bcast:15 -> rows 1, 3
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, false));      // row_bcast:31 -> rows 2, 3
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float pr_uniform(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// one cell with PA active pairs (bins 0 .. 128 PA - 1)
template <int PA, int NP>
__device__ __forceinline__ void pr_step(pr_f2 (&c)[NP], const pr_f2 (&e)[NP], const float* us, float* zs, float* pzs, int i, int HW, int lane,
                                        float& unext, int& seen) {
    const float u = pr_uniform(unext);
    unext = us[min(i + 1, HW - 1)];
    // q_j = j * (1 / rem); 1 / rem rounded up when rem * (1 / rem) < 1 (exact test through the fma): the product at j = rem is then >= 1
    // and the clamp makes it exactly 1
    const float rem = (float)(HW - i), r0 = pr_rcp(rem);
    const float inv_rem = fmaf(rem, r0, -1.f) < 0.f ? __builtin_bit_cast(float, __builtin_bit_cast(int, r0) + 1) : r0;
    const pr_f2 ir2 = {inv_rem, inv_rem}, one2 = {1.f, 1.f};
    pr_f2 von[PA], voff[PA], s_on = {0.f, 0.f}, s_off = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < PA; ++k) {
        pr_f2 q = e[k] * ir2;
        if (k == PA - 1) { q.x = fminf(q.x, 1.f); q.y = fminf(q.y, 1.f); }      // the last active pair: bins at and past `rem`
        von[k] = c[k] * q;
        voff[k] = c[k] * (one2 - q);
        s_on += von[k];
        s_off += voff[k];
    }
    const float pz = pr_wave_sum(s_on.x + s_on.y);
    const float n_off = pr_wave_sum(s_off.x + s_off.y);
    const bool on = u < pz;                           // wave-uniform
    const float inv_np = pr_rcp(fmaxf(on ? pz : n_off, 1e-6f));
    const pr_f2 in2 = {inv_np, inv_np};
#pragma unroll
    for (int k = 0; k < PA; ++k) c[k] = (on ? von[k] : voff[k]) * in2;
    if (lane == 0) { zs[i] = on ? 1.f : 0.f; pzs[i] = fminf(pz, 1.f); }
    if (on) {                                         // every bin moves down by one (bin 0, now empty, drops out)
        ++seen;
        // wave rotate by one lane (DPP): r[l] = v[l + 1], r[63] = v[0] -- so lane 63 of a register's new value is lane 63 of the NEXT
        // register's rotation; one DPP move and one select per register, no lane reads through scalar registers
        auto rol1 = [](float v) {
            return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x134, 0xf, 0xf, false));
        };
        const bool top = lane == 63;
        float r[2 * PA + 1];
#pragma unroll
        for (int k = 0; k < PA; ++k) { r[2 * k] = rol1(c[k].x); r[2 * k + 1] = rol1(c[k].y); }
        r[2 * PA] = 0.f;
#pragma unroll
        for (int k = 0; k < PA; ++k) {
            c[k].x = top ? r[2 * k + 1] : r[2 * k];
            c[k].y = top ? r[2 * k + 2] : r[2 * k + 1];
        }
    }
}
// the steps with floor((HW - i) / 128) + 1 == PA, then the phases below
template <int PA, int NP>
__device__ __forceinline__ void pr_phase(pr_f2 (&c)[NP], const pr_f2 (&e)[NP], const float* us, float* zs, float* pzs, int HW, int lane,
                                         float& unext, int& seen) {
    const int lo = max(0, HW - 128 * PA + 1), hi = min(HW - 1, HW - 128 * (PA - 1));
    for (int i = lo; i <= hi; ++i) pr_step<PA, NP>(c, e, us, zs, pzs, i, HW, lane, unext, seen);
    if constexpr (PA > 1) pr_phase<PA - 1, NP>(c, e, us, zs, pzs, HW, lane, unext, seen);
}

template <int NP, int WPB>
__global__ __launch_bounds__(WPB * 64) void k_prior_presence(const float* __restrict__ u, int B, int HW, float prior_prob,
                                                             const int* __restrict__ count, float* __restrict__ z_pres,
                                                             float* __restrict__ p_z, int* __restrict__ n_present) {
    extern __shared__ float pr_sh[];          // [WPB][3][HW]: u, z_pres, p_z of the wave's sample
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * WPB + wave;
    if (b >= B) return;                       // (no workgroup barrier below)
    float* us = pr_sh + (size_t)wave * 3 * HW;
    float* zs = us + HW;
    float* pzs = zs + HW;
    const size_t row = (size_t)b * HW;
    for (int i = lane; i < HW; i += 64) us[i] = u[row + i];
    wave_lds_fence();
    int seen = 0;
    if (count) {
        // one-hot at n: need / rem in integers, the quotient correctly rounded
        int need = min(max(count[b], 0), HW);
        need = __builtin_amdgcn_readfirstlane(need);
        for (int i = 0; i < HW; ++i) {
            const int rem = HW - i;
            const float pz = __fdiv_rn((float)need, (float)rem);
            const float ui = pr_uniform(us[i]);
            const bool on = need >= rem || (need > 0 && ui < pz);
            if (lane == 0) { zs[i] = on ? 1.f : 0.f; pzs[i] = pz; }
            need -= on ? 1 : 0;
            seen += on ? 1 : 0;
        }
    } else {
        // geometric count distribution (1 - p) p^c, c = 0 .. HW, normalised (models.py:190-193); bins past HW stay 0
        pr_f2 c[NP], e[NP];
        float part = 0.f;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int j0 = 2 * k * 64 + lane, j1 = j0 + 64;
            e[k] = pr_f2{(float)j0, (float)j1};
            c[k].x = j0 <= HW ? (1.f - prior_prob) * powf(prior_prob, (float)j0) : 0.f;
            c[k].y = j1 <= HW ? (1.f - prior_prob) * powf(prior_prob, (float)j1) : 0.f;
            part += c[k].x + c[k].y;
        }
        const float norm0 = pr_wave_sum(part);
#pragma unroll
        for (int k = 0; k < NP; ++k) { c[k].x = c[k].x / norm0; c[k].y = c[k].y / norm0; }
        float unext = us[0];
        pr_phase<NP, NP>(c, e, us, zs, pzs, HW, lane, unext, seen);
    }
    wave_lds_fence();
    for (int i = lane; i < HW; i += 64) { z_pres[row + i] = zs[i]; p_z[row + i] = pzs[i]; }
    if (lane == 0) n_present[b] = seen;
}

__global__ __launch_bounds__(256) void k_prior_gauss(CellHyper H, int B, int A, int G, int Gw, const float* __restrict__ eps_box,
                                                     const float* __restrict__ eps_attr, const float* __restrict__ eps_depth,
                                                     float* __restrict__ z_where, float* __restrict__ z_what, float* __restrict__ z_depth) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int HW = G * Gw, CH = A + 5;
    if (idx >= (long long)B * CH * HW) return;
    const int cell = (int)(idx % HW);
    const long long t = idx / HW;
    const int ch = (int)(t % CH), b = (int)(t / CH);
    if (ch < 4) {
        const float* eb = eps_box + (size_t)b * 4 * HW + cell;
        float lat[8];
        const float zero[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) { lat[k] = H.prior_mean[k] + H.prior_std[k] * eb[(size_t)k * HW]; lat[4 + k] = 0.f; }
        const BoxFwd o = box_forward(lat, zero, H, cell / Gw, cell % Gw);
        z_where[((size_t)b * 4 + ch) * HW + cell] = ch == 0 ? o.nbox[0] : ch == 1 ? o.nbox[1] : ch == 2 ? o.nbox[2] : o.nbox[3];
    } else if (ch < 4 + A) {
        const size_t o = ((size_t)b * A + (ch - 4)) * HW + cell;
        z_what[o] = H.prior_mean[4] + H.prior_std[4] * eps_attr[o];
    } else {
        const size_t o = (size_t)b * HW + cell;
        float mu, sd, depth;
        depth_forward(H.prior_mean[5] + H.prior_std[5] * eps_depth[o], 0.f, 0.f, H, mu, sd, depth);
        z_depth[o] = depth;
    }
}

bool prob_ok(float p) { return p > 0.f && p < 1.f; }      // (false for NaN)

}  // namespace

int prior_presence(const float* u, int B, int HW, float prior_prob, const int* count, float* z_pres, float* p_z, int* n_present,
                   hipStream_t s) {
    if (!u || !z_pres || !p_z || !n_present || B < 1 || HW < 1 || HW > PRIOR_MAX_HW) return SPAIR_ERR_SHAPE;
    if (!count && !prob_ok(prior_prob)) return SPAIR_ERR_SHAPE;
    constexpr int W = 4;       // samples per workgroup: one wave per SIMD, as k_count_kl runs
    const dim3 grid(ceil_div(B, W)), block(W * 64);
    const size_t lds = (size_t)W * 3 * HW * sizeof(float);      // <= 48 KB
#define SP_PRIOR_LAUNCH(NP_) \
    hipLaunchKernelGGL((k_prior_presence<NP_, W>), grid, block, lds, s, u, B, HW, prior_prob, count, z_pres, p_z, n_present)
    if (HW + 1 <= 2 * 64) SP_PRIOR_LAUNCH(1);
    else if (HW + 1 <= 6 * 64) SP_PRIOR_LAUNCH(3);
    else if (HW + 1 <= 10 * 64) SP_PRIOR_LAUNCH(5);
    else SP_PRIOR_LAUNCH(9);
#undef SP_PRIOR_LAUNCH
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}

int prior_gauss_maps(const CellHyper& H, int B, int A, int G, int Gw, const float* eps_box, const float* eps_attr, const float* eps_depth,
                     float* z_where, float* z_what, float* z_depth, hipStream_t s) {
    const long long total = (long long)B * (A + 5) * G * Gw;
    if (total > 0x7fffffffLL * 256) return SPAIR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_prior_gauss, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, H, B, A, G, Gw, eps_box, eps_attr, eps_depth,
                       z_where, z_what, z_depth);
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}

extern "C" int spair_prior_presence(const float* u, int B, int HW, float count_prior_prob, const int* count, float* z_pres, float* p_z,
                                    int* n_present, void* stream) {
    return prior_presence(u, B, HW, count_prior_prob, count, z_pres, p_z, n_present, (hipStream_t)stream);
}

// The priors and box ranges of `d` as the step's CellHyper carries them (engine.hip, ctx_init); both kernels on the caller's stream, no
// workspace, no status word.  Everything is checked before the first launch.
extern "C" int spair_prior_sample(const SpairDims* d0, float count_prior_prob, const int* count, const float* eps_box, const float* eps_attr,
                                  const float* eps_depth, const float* u_pres, float* z_where, float* z_what, float* z_depth, float* z_pres,
                                  float* p_z, int* n_present, void* stream) {
    if (!d0 || !eps_box || !eps_attr || !eps_depth || !u_pres || !z_where || !z_what || !z_depth || !z_pres || !p_z || !n_present)
        return SPAIR_ERR_SHAPE;
    const SpairDims dn = spair_dims_norm(*d0), *d = &dn;
    if (d->B < 1 || d->G < 1 || d->Gw < 1 || d->A < 1 || d->I < 1 || d->Iw < 1 || d->cell_px < 1) return SPAIR_ERR_SHAPE;
    if ((long long)d->G * d->Gw > PRIOR_MAX_HW) return SPAIR_ERR_SHAPE;
    if (!count && !prob_ok(count_prior_prob)) return SPAIR_ERR_SHAPE;
    CellHyper H;
    H.wheel = 0.f; H.kl_scale = 0.f; H.img = (float)d->I; H.anchor = d->anchor;
    H.cell_over_img = (float)((double)d->cell_px / (double)d->I);
    H.img_w = (float)d->Iw;
    H.cell_over_w = (float)((double)d->cell_px / (double)d->Iw);
    H.max_yx = d->max_yx; H.min_yx = d->min_yx; H.max_hw = d->max_hw; H.min_hw = d->min_hw;
    H.range_yx = d->max_yx - d->min_yx; H.range_hw = d->max_hw - d->min_hw;
    for (int i = 0; i < 6; ++i) { H.prior_mean[i] = d->prior_mean[i]; H.prior_std[i] = d->prior_std[i]; }
    H.count_prior_prob = count_prior_prob;
    const hipStream_t s = (hipStream_t)stream;
    const int rc = prior_gauss_maps(H, d->B, d->A, d->G, d->Gw, eps_box, eps_attr, eps_depth, z_where, z_what, z_depth, s);
    if (rc != SPAIR_OK) return rc;
    return prior_presence(u_pres, d->B, d->G * d->Gw, count_prior_prob, count, z_pres, p_z, n_present, s);
}
