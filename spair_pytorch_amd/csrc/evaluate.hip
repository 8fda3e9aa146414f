// SPAIR.evaluate: the loss of one forward per image, per cell and per pixel (reference: _compute_KL models.py:169-262, _build_loss :544-563).
//   k_sample_terms        : grid B x S.  Workgroup (b, s) takes slice s of sample b's cells and slice s of its pixels, writes their
//                           kl_map / bce_map elements and ONE partial of 8 sums (BCE, six Gaussian KLs, presence KL) to scratch.
//   k_sample_terms_finish : one wave per sample adds its S partials in a fixed order -> terms [B][9].
// The training step reduces the same operands across samples (k_gauss_kl blocks take rows r = cell * B + b, bce_partial is laid out per
// renderer family), so nothing per image can be recovered from its partials: this reads the STORED operands of the forward again.
// No atomics; every output element has one writer and every sum a fixed order: bit-identical from run to run.
//
// Cells: one wave per row in k_gauss_kl's lane layout (lane j < A the attribute element j, lanes A .. A+3 the box latents, lane A+4 the
// depth): coalesced row reads, no index arithmetic.  z_pres and p_z of the row are wave-uniform loads; every lane forms the presence term
// (A = 59 fills all 64 lanes: it has no lane of its own), lane 0 stores it.
// Pixels: a lane takes four consecutive pixels of every channel, 16 bytes per load, where every image plane starts 16-byte aligned
// (I * Iw a multiple of 4 and aligned bases; VEC); otherwise one pixel per lane, consecutive lanes on consecutive pixels.  A slice's share
// is a whole number of those units, so the last slice's tail is the loop bound, not a special case.
//
// The split (eval_slices): a sample's work is HW rows (a wave each) and C * I * Iw pixels; one workgroup per sample leaves B workgroups of
// dependent reductions on 256 CUs (B = 1 with 1024 cells: one CU).  S = ceil(2048 / B) workgroups per sample -- 8 resident workgroups of
// 256 threads on each of the 256 CUs in a single round -- but never more than gives every workgroup one row per wave or four pixels per
// lane (a smaller slice only adds partials), and at most EVAL_MAX_SLICES.
#include <algorithm>
#include "evaluate.h"

namespace {

#define EVAL_TARGET_BLOCKS 2048

__device__ __forceinline__ float ev_gauss(float mu, float sd, float m, float s) {
    const float vr = (sd / s) * (sd / s);
    const float t1 = ((mu - m) / s) * ((mu - m) / s);
    return 0.5f * (vr + t1 - 1.f - logf(vr));
}
// torch's binary_cross_entropy: both logs clamped at -100
__device__ __forceinline__ float ev_bce(float r, float xv) {
    return -(xv * fmaxf(logf(r), -100.f) + (1.f - xv) * fmaxf(logf(1.f - r), -100.f));
}
// map = (accumulate ? map : 0) + scale * value; the old value is only read when it is asked for
__device__ __forceinline__ void ev_put(float* p, float v, int accumulate, float scale) {
    *p = (accumulate ? *p : 0.f) + scale * v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_sample_terms(EvalRows R, int B, int HW, int A, int C, long long npix, int S, int cells_per,
                                                      long long units_per, const float* __restrict__ recon, const float* __restrict__ x,
                                                      float* __restrict__ part, float* __restrict__ kl_map, float* __restrict__ bce_map,
                                                      int accumulate, float scale) {
    __shared__ float red[4][EVAL_NPART];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x / S, s = blockIdx.x - b * S;
    // ---- cells k0 .. k1-1: a wave per row ----
    const int kind = lane < A ? 4 : lane < A + 4 ? lane - A : lane == A + 4 ? 5 : -1;
    const float pm = kind >= 0 ? R.prior_mean[kind] : 0.f, ps = kind >= 0 ? R.prior_std[kind] : 1.f;
    float acc = 0.f, accp = 0.f;
    const int k0 = s * cells_per, k1 = min(HW, k0 + cells_per);
    for (int k = k0 + wave; k < k1; k += 4) {
        const size_t r = (size_t)(R.cidx ? R.cidx[k] : k) * B + b;
        const float z = R.z_pres[r * R.ld_z], pz = R.p_z[r * R.ld_pz];
        float mu = pm, sd = ps;                                                              // (idle lanes: KL = 0)
        if (kind == 4) { mu = R.mu_attr[r * R.ld_mu_attr + lane]; sd = R.sd_attr[r * R.ld_sd_attr + lane]; }
        else if (kind == 5) { mu = R.mu_depth[r * R.ld_mu_depth]; sd = R.sd_depth[r * R.ld_sd_depth]; }
        else if (kind >= 0) { mu = R.mu_box[r * R.ld_mu_box + kind]; sd = R.sd_box[r * R.ld_sd_box + kind]; }
        const float v = z * ev_gauss(mu, sd, pm, ps);
        const float e9 = 1e-9f;
        const float vp = z * (logf(z + e9) - logf(pz + e9)) + (1.f - z) * (logf(1.f - z + e9) - logf(1.f - pz + e9));
        acc += v;
        accp += vp;
        if (kl_map) {                                                                        // (wave-uniform)
            const float attr = wave_reduce_sum(kind == 4 ? v : 0.f);
            float* m = kl_map + (size_t)b * 7 * HW + k;
            if (kind >= 0 && kind != 4) ev_put(m + (size_t)kind * HW, v, accumulate, scale);
            if (lane == 0) {
                ev_put(m + (size_t)4 * HW, attr, accumulate, scale);
                ev_put(m + (size_t)6 * HW, vp, accumulate, scale);
            }
        }
    }
    // ---- pixels: units u0 .. u1-1 of the plane (VEC: four pixels each) ----
    float bce = 0.f;
    const long long nunits = VEC ? npix / 4 : npix;
    const long long u0 = (long long)s * units_per, u1 = u0 + units_per < nunits ? u0 + units_per : nunits;
    const size_t img = (size_t)b * C * (size_t)npix;
    for (long long u = u0 + threadIdx.x; u < u1; u += 256) {
        if constexpr (VEC) {
            f32x4 sum = {0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < C; ++c) {
                const size_t o = img + (size_t)c * (size_t)npix + 4 * (size_t)u;
                const f32x4 rv = *reinterpret_cast<const f32x4*>(recon + o), xv = *reinterpret_cast<const f32x4*>(x + o);
                sum.x += ev_bce(rv.x, xv.x); sum.y += ev_bce(rv.y, xv.y); sum.z += ev_bce(rv.z, xv.z); sum.w += ev_bce(rv.w, xv.w);
            }
            bce += (sum.x + sum.y) + (sum.z + sum.w);
            if (bce_map) {
                f32x4* m = reinterpret_cast<f32x4*>(bce_map + (size_t)b * (size_t)npix + 4 * (size_t)u);
                f32x4 old = {0.f, 0.f, 0.f, 0.f};
                if (accumulate) old = *m;
                *m = old + scale * sum;
            }
        } else {
            float sum = 0.f;
            for (int c = 0; c < C; ++c) {
                const size_t o = img + (size_t)c * (size_t)npix + (size_t)u;
                sum += ev_bce(recon[o], x[o]);
            }
            bce += sum;
            if (bce_map) ev_put(bce_map + (size_t)b * (size_t)npix + (size_t)u, sum, accumulate, scale);
        }
    }
    // ---- this workgroup's partial: every slot of red[wave] has exactly one writer ----
    bce = wave_reduce_sum(bce);
    const float attr = wave_reduce_sum(kind == 4 ? acc : 0.f);
    if (kind >= 0 && kind != 4) red[wave][kind < 4 ? 1 + kind : 6] = acc;
    if (lane == 0) { red[wave][0] = bce; red[wave][5] = attr; red[wave][7] = accp; }
    __syncthreads();
    if (threadIdx.x < EVAL_NPART)
        part[(size_t)blockIdx.x * EVAL_NPART + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// terms[b] = (BCE + beta * sum of the seven KLs, BCE, KL cy, cx, height, width, attr, depth, presence): lane l adds partials l, l + 64, ...
// then the wave's fixed reduction tree
__global__ __launch_bounds__(256) void k_sample_terms_finish(const float* __restrict__ part, int B, int S, float beta, float* __restrict__ terms) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                                                      // (a whole wave)
    float t[EVAL_NPART];
#pragma unroll
    for (int j = 0; j < EVAL_NPART; ++j) {
        float v = 0.f;
        for (int s = lane; s < S; s += 64) v += part[((size_t)b * S + s) * EVAL_NPART + j];
        t[j] = wave_reduce_sum(v);
    }
    if (lane == 0) {
        float kl = 0.f;
#pragma unroll
        for (int j = 1; j < EVAL_NPART; ++j) { terms[(size_t)b * 9 + 1 + j] = t[j]; kl += t[j]; }
        terms[(size_t)b * 9 + 1] = t[0];
        terms[(size_t)b * 9] = t[0] + beta * kl;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int eval_slices(int B, int HW, long long npix) {
    const long long by_work = std::max<long long>((HW + 3) / 4, (npix + 1023) / 1024);
    const long long want = (EVAL_TARGET_BLOCKS + (long long)B - 1) / B;
    return (int)std::max<long long>(1, std::min<long long>(std::min<long long>(want, by_work), EVAL_MAX_SLICES));
}
long long eval_scratch_floats(int B, int HW, long long npix) { return (long long)B * eval_slices(B, HW, npix) * EVAL_NPART; }

int eval_sample_terms(const EvalRows& R, int B, int HW, int A, int C, int I, int Iw, float beta, const float* recon, const float* x,
                      float* terms, float* kl_map, float* bce_map, float* scratch, int accumulate, float scale, hipStream_t s) {
    if (B < 1 || HW < 1 || HW > EVAL_MAX_HW || A < 1 || A + 5 > 64 || C < 1 || I < 1 || Iw < 1) return SPAIR_ERR_SHAPE;
    if (!R.z_pres || !R.p_z || !R.mu_box || !R.sd_box || !R.mu_attr || !R.sd_attr || !R.mu_depth || !R.sd_depth) return SPAIR_ERR_SHAPE;
    if (!recon || !x || !terms || !scratch) return SPAIR_ERR_SHAPE;
    if (R.ld_z < 1 || R.ld_pz < 1 || R.ld_mu_box < 4 || R.ld_sd_box < 4 || R.ld_mu_attr < A || R.ld_sd_attr < A || R.ld_mu_depth < 1 ||
        R.ld_sd_depth < 1)
        return SPAIR_ERR_SHAPE;
    const long long npix = (long long)I * Iw;
    const int S = eval_slices(B, HW, npix);
    if ((long long)B * S > 0x7fffffffLL) return SPAIR_ERR_UNSUPPORTED;
    const bool vec = npix % 4 == 0 && aligned16(recon) && aligned16(x) && (!bce_map || aligned16(bce_map));
    const long long nunits = vec ? npix / 4 : npix;
    const int cells_per = ceil_div(HW, S);
    const long long units_per = (nunits + S - 1) / S;
    const dim3 grid((unsigned)(B * S)), block(256);
    if (vec)
        hipLaunchKernelGGL((k_sample_terms<true>), grid, block, 0, s, R, B, HW, A, C, npix, S, cells_per, units_per, recon, x, scratch, kl_map,
                           bce_map, accumulate, scale);
    else
        hipLaunchKernelGGL((k_sample_terms<false>), grid, block, 0, s, R, B, HW, A, C, npix, S, cells_per, units_per, recon, x, scratch, kl_map,
                           bce_map, accumulate, scale);
    SPAIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sample_terms_finish, dim3(ceil_div(B, 4)), dim3(256), 0, s, scratch, B, S, beta, terms);
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}

// ---- C ABI (include/spair_hip.h, "evaluation") --------------------------------------------------------------------------------------------
extern "C" long long spair_sample_terms_scratch_floats(int B, int HW, int I, int Iw) {
    if (B < 1 || HW < 1 || HW > EVAL_MAX_HW || I < 1 || Iw < 1) return SPAIR_ERR_SHAPE;
    return eval_scratch_floats(B, HW, (long long)I * Iw);
}

extern "C" int spair_sample_terms_rows(const float* z_pres, int ld_z, const float* p_z, int ld_pz, const float* mu_box, int ld_mu_box,
                                       const float* sd_box, int ld_sd_box, const float* mu_attr, int ld_mu_attr, const float* sd_attr,
                                       int ld_sd_attr, const float* mu_depth, int ld_mu_depth, const float* sd_depth, int ld_sd_depth,
                                       const int* cidx, const float* prior_mean, const float* prior_std, float beta, const float* recon,
                                       const float* x, int B, int HW, int A, int C, int I, int Iw, float* terms, float* kl_map,
                                       float* bce_map, float* scratch, int accumulate, float scale, void* stream) {
    if (!prior_mean || !prior_std) return SPAIR_ERR_SHAPE;
    EvalRows R;
    R.z_pres = z_pres; R.p_z = p_z; R.mu_box = mu_box; R.sd_box = sd_box; R.mu_attr = mu_attr; R.sd_attr = sd_attr;
    R.mu_depth = mu_depth; R.sd_depth = sd_depth;
    R.ld_z = ld_z; R.ld_pz = ld_pz; R.ld_mu_box = ld_mu_box; R.ld_sd_box = ld_sd_box; R.ld_mu_attr = ld_mu_attr; R.ld_sd_attr = ld_sd_attr;
    R.ld_mu_depth = ld_mu_depth; R.ld_sd_depth = ld_sd_depth;
    R.cidx = cidx;
    for (int i = 0; i < 6; ++i) { R.prior_mean[i] = prior_mean[i]; R.prior_std[i] = prior_std[i]; }
    return eval_sample_terms(R, B, HW, A, C, I, Iw, beta, recon, x, terms, kl_map, bce_map, scratch, accumulate, scale, (hipStream_t)stream);
}
