/* libspair_hip.so -- C ABI of the MI355X-native SPAIR training step.
 *
 * This is the drop-in boundary beneath the Python surface `spair_pytorch_amd.models.SPAIR`
 * (which mirrors /root/reference/spair/models.py:15-131).  The reference has no FFI layer of
 * its own: what these entry points replace is the ATen/cuDNN/cuBLAS work its forward/backward
 * dispatches (SURVEY.md §2 "Library-op inventory").  Conventions:
 *   - every pointer is a DEVICE pointer into caller-owned memory; nothing is allocated or freed,
 *     scratch is passed in explicitly (`workspace`, zero-initialised ONCE by the caller: the
 *     library relies on never-written pad columns staying zero);
 *   - work is enqueued on `stream` (a hipStream_t) and never synchronises;
 *   - return 0 on success, a negative SPAIR_ERR_* code otherwise (shape / dtype / launch);
 *   - all step state lives in the buffers the caller passes.  The only library-owned objects are one low-priority helper HIP stream
 *     (+ 6 fork/join events) per device, created under a lock on first use or by spair_init(), and the opt-in profiling event pool
 *     (spair_prof_*, lock-protected, off by default).  Calls on different devices or different caller streams may be issued concurrently
 *     from different host threads as long as they use different workspaces: the fork/join events are per device, so each
 *     spair_forward / spair_backward holds that device's enqueue lock from its first fork to its last join (host-side only -- the
 *     enqueued work of the two callers still overlaps on the GPU; tests/test_surface_gpu.py drives two models from two threads).
 *     Create the helper stream with spair_init() before capturing a step into a hipGraph.
 */
#pragma once
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SPAIR_DTYPE_F32 0   /* GEMM/conv operands fp32 (v_mfma_f32_16x16x4_f32), exact */
#define SPAIR_DTYPE_BF16 1  /* GEMM/conv operands bf16, fp32 accumulate (v_mfma_f32_16x16x32_bf16) */

/* Hyper-parameters = /root/reference/spair/config.py:3-76 plus the batch geometry. */
typedef struct SpairDims {
    int B, C, I, G;            /* batch, image channels (config.py:4 INPUT_IMAGE_SHAPE[0]: 1 = the benchmarked fused kernels; 2, 3 = colour
                                * images on the per-wavefront launches with the generic-channel renderer, either dtype), image side, grid side */
    int P, A, F, NP;           /* OBJECT_SHAPE[0], N_ATTRIBUTES, N_BACKBONE_FEATURES, N_PASSTHROUGH_FEATURES */
    int n_conv;                /* backbone conv layers before conv_out (config.py:7-14) */
    int conv_k[8], conv_s[8], conv_c[8];
    int pad_pre, pad_post, cell_px;   /* receptive-field padding (modules.py:68-105) */
    int dtype;                 /* SPAIR_DTYPE_* */
    int align_corners;         /* 0 = torch>=1.3 default (the pinned oracle), 1 = torch 1.0 era */
    float anchor;              /* ANCHORBOX_SHAPE[0] */
    float max_yx, min_yx, max_hw, min_hw;
    float obj_logit_scale, alpha_logit_scale, alpha_logit_bias;
    float vae_beta;            /* VAE_BETA (config.py:55) */
    float prior_mean[6], prior_std[6];   /* cy, cx, height, width, attr, depth (config.py:45-52) */
    /* Convolutional object encoder / decoder variant (CONV_OBJECT_ENCODER_TOPOLOGY, config.py:15-20; models.py:606-665 sketches the two
     * classes but cannot run them: PARITY UNPINNED).  obj_conv = 1 replaces the MLP encoder by oc_n valid convolutions (filters oc_c,
     * kernel oc_k, stride oc_s, ReLU after each) + Linear(flattened (C,H,W) -> 2A), and the MLP decoder by Linear(A -> flattened) + the
     * mirrored ConvTranspose2d stack (output_padding retraces the encoder's sizes; ReLU between, none after the last; its C+1 output
     * channels are the sprite's (colour.., alpha) logits).  Per-wavefront launches in either dtype; the convolutions themselves and the
     * sprites they produce are fp32 (the bf16 step keeps bf16 GEMM operands for the backbone, the other per-cell nets and the two Linears).  Parameter
     * names: object_encoder.conv.conv_<i>.{weight,bias}, object_encoder.out.*, object_decoder.inp.*,
     * object_decoder.conv.conv_transposed_<i>.* (ConvTranspose2d layout [in][out][k][k]). */
    int obj_conv, oc_n;
    int oc_k[4], oc_s[4], oc_c[4];
    /* N_LOOKBACK (config.py:31, models.py:292-320): a cell's lateral context is the 2L(L+1) already-visited cells of rows h-L..h,
     * columns w-L..w+L, in the reference's order (row-major, the current cell and those to its right dropped); out-of-grid slots read
     * the learned edge element.  0 is read as 1 (the reference's configuration: UL, U, UR, L).  L != 1 runs on the per-wavefront
     * launches (dependency wavefronts t = (L+1) h + w); the fused per-cell kernels are built for L = 1.  1 <= L <= 3. */
    int lookback;
    /* Rectangular images (appended; 0 = "same as the square fields", so a zero-initialised tail keeps the square meaning).  With them I, G
     * and pad_post are the HEIGHT axis: the image is I x Iw pixels, the grid Gh x Gw = G x Gw cells, the padded frame
     * (pad_pre + I + pad_post) x (pad_pre + Iw + pad_post_w).  pad_pre and cell_px are shared (square kernels and strides).  A rectangular
     * image (Iw != I) runs on the per-wavefront launches, the implicit-GEMM / per-class backbone convolutions and the first-generation
     * (grey) or generic-channel (colour) renderer: the kernel plan refuses every square-only specialisation.  G * Gw + 1 <= 1025;
     * lookback > 1 needs max(G, Gw) <= 32. */
    int Iw, Gw, pad_post_w;
} SpairDims;

/* Version of the layouts of SpairDims, SpairStep and SpairStepIO (and of the entry points' argument lists): a binding checks it before it
 * passes a struct. */
#define SPAIR_ABI_VERSION 3
int spair_abi_version(void);

/* Per-step scalars (host side evaluates the two schedules, modules.py:191-213). */
typedef struct SpairStep {
    float wheel;               /* LATENT_VAR_TRAINING_WHEEL value */
    float count_prior_prob;    /* 1/(1+exp(-log(v+1e-6))), models.py:186-188 */
    float kl_scale;            /* 1/(B*world_size): batch-mean of the KL terms (models.py:553) */
    int train;                 /* 1: keep what backward needs */
    int flags;                 /* bits 0 and 2-6 are inputs of the step's kernel plan (spair_step_plan); bit 1 is not.
                                * bit 0: disable the fused persistent per-cell kernels (A/B testing); bit 1: record stage stamps;
                                * bit 2: no helper stream (every kernel on the caller's stream);
                                * bit 3: stem weight gradient as its own kernel (not fused into conv_1's data gradient);
                                * bit 4: decoder forward as three GEMM launches instead of the fused activation-stationary kernel;
                                * bit 5: strided backbone convs through the implicit-GEMM kernel instead of the patch-resident one;
                                * bit 6: decoder data gradients as three GEMM launches instead of the fused kernel */
    int draw_noise;            /* spair_forward only: 1 = fill SpairStepIO's four noise maps from noise_seed first (what spair_noise_fill
                                * does, but on the helper stream beside the backbone) */
    unsigned long long noise_seed;
    /* Non-finite / failed steps made loud without a host synchronisation (the reference RAISES on any NaN in its forward:
     * spair/debug_tools.py:245-271, called at models.py:65,108,245).  spair_forward's loss kernel evaluates
     *   bits = 1 * (a band-split hand-off of the per-cell chain ever timed out on this workspace) | 2 * (a loss term of THIS forward is NaN / inf)
     * and, where the pointers are non-null, writes
     *   status[0] |= bits (sticky)   -- two ints in device memory, caller-owned;
     *   status[1] |= bits, only with train != 0   -- the word of the OPTIMIZER step (spair_adam_guarded's skip word): every train forward
     *   since it was last cleared has ORed into it (micro-batches of one accumulated step), a forward with train == 0 leaves it alone (an
     *   evaluation between backward and optimizer step changes nothing).  Whoever applies the step clears it afterwards (FusedAdam.step
     *   does; hipMemsetAsync of the one int behind spair_adam_guarded in a C caller);
     *   *status_host = bits, only when bits != 0   -- one int of host memory the device can write (spair_host_word_alloc), so that the
     *   caller can poll it with a plain load at any later point (a normal step never touches it).  Both may be NULL. */
    int* status;
    int* status_host;
} SpairStep;

/* Optional: create the current device's helper stream now (otherwise on the first spair_forward / spair_backward). */
int spair_init(void);

/* ---- parameter / workspace layout -------------------------------------------------------- */
/* Flat fp32 parameter buffer; tensor i of the reference state_dict (same key, same shape). */
int spair_param_count(const SpairDims* d);
int spair_param_info(const SpairDims* d, int idx, char* name, int name_cap, int64_t* offset, int64_t* shape4, int* ndim);
int64_t spair_param_total(const SpairDims* d);
int64_t spair_workspace_bytes(const SpairDims* d);

/* ---- the training step ---------------------------------------------------------------------
 * forward  == SPAIR.forward (models.py:35-131): backbone -> per-cell loop -> KL -> render -> loss.
 * backward == loss.backward() (train.py:66): accumulates into `grads` (same layout as params).
 * Both take the step's device memory in one SpairStepIO.  An optional field may be NULL: that part of the step is left out and launches
 * nothing, so a backward with every optional field NULL is the plain backward, kernel for kernel.  Maps are NCHW. */
typedef struct SpairStepIO {
    /* read by both directions: the backward takes the buffers of the forward (SpairStep.train = 1) it follows.  None may be NULL. */
    const float* params;       /* flat fp32 parameters (spair_param_info) */
    const float* x;            /* input image [B,C,I,Iw] */
    float* eps_box;            /* noise maps: [B,4,G,Gw] (cy,cx,height,width), */
    float* eps_attr;           /*   [B,A,G,Gw], */
    float* eps_depth;          /*   [B,1,G,Gw], */
    float* u_pres;             /*   [B,1,G,Gw]; spair_forward writes all four first when SpairStep.draw_noise is set */
    void* workspace;           /* spair_workspace_bytes(d) bytes, zeroed once by the caller */
    /* spair_forward */
    float* loss_out;           /* >= 10 floats: [0]=total, [1]=BCE sum, [2..8]=KL cy,cx,height,width,attr,depth,pres (batch means), [9]=total
                                * again (a second copy for a host layer that hands the loss out as a view: an in-place op on it then leaves
                                * the logged terms [0..8] alone) */
    float* recon;              /* [B,C,I,Iw] */
    float* z_where;            /* [B,4,G,Gw] */
    float* z_pres;             /* [B,1,G,Gw] */
    float* inv_den;            /* optional: [B][I][Iw], 1/D of the renderer's composite per pixel, kept for a backward with grad_recon */
    /* spair_backward */
    const float* grad_loss;    /* one float; may point at a zero for a backward through the outputs alone */
    float* grads;              /* accumulated into */
    /* Data-parallel hook (the reference is single-device, train.py:27-30): the backward completes the gradients in three
     * contiguous ranges of `grads` (spair_grad_buckets) in this order.  Optional caller-created hipEvent_t, recorded when its range is
     * final, so that its all-reduce can overlap the rest. */
    void* ev_decoder;          /* decoder */
    void* ev_cells;            /* box / encoder / z / obj nets */
    void* ev_backbone;         /* edge element + backbone */
    /* Differentiable outputs (the reference returns recon, z_where and z_pres as autograd tensors, models.py:35-131, so a user term on any
     * of them trains through the model).  Optional adjoints of the three outputs, folded into the reverse pass element for element, no
     * atomics: deterministic. */
    const float* grad_recon;   /* [B,C,I,Iw]: needs the inv_den of the same forward and aux_scratch, else SPAIR_ERR_SHAPE */
    const float* grad_z_where; /* [B,4,G,Gw] */
    const float* grad_z_pres;  /* [B,1,G,Gw] */
    float* aux_scratch;        /* 2*B*C*I*Iw + 1 floats, only touched with grad_recon (the workspace keeps what the forward saved, so a
                                * second backward through the same forward is unaffected) */
    /* Optional: the gradient of the step with respect to its input image, OVERWRITTEN, fp32 [B,C,I,Iw]: the backbone term (the stem's data
     * gradient from d act0), the glimpse term (the adjoint of the border-padded STN glimpse) and, with bce_target != 0, the BCE-target term
     * *grad_loss * (log1p(-recon) - log(recon)) -- torch's gradient of binary_cross_entropy with respect to its target, not clamped: +inf
     * where recon == 0, -inf where recon == 1 (the status word is not affected).  Its kernels run after ev_backbone is recorded; no atomics
     * on grad_x: deterministic.  SPAIR_ERR_UNSUPPORTED for fewer than 2 backbone layers or a stem of more than 64 KiB of weights. */
    float* grad_x;
    void* x_scratch;           /* spair_input_grad_scratch_bytes(d) bytes: needed with grad_x, else SPAIR_ERR_SHAPE */
    int bce_target;            /* with grad_x; 0 is for a backward through the outputs alone, where the loss is not part of the graph */
} SpairStepIO;
int spair_forward(const SpairDims* d, const SpairStep* st, const SpairStepIO* io, void* stream);
int spair_backward(const SpairDims* d, const SpairStep* st, const SpairStepIO* io, void* stream);
/* the three ranges of SpairStepIO.ev_*, as element offsets [lo, hi) into `grads` */
int spair_grad_buckets(const SpairDims* d, int64_t* lo3, int64_t* hi3);
/* host arithmetic only: bytes of SpairStepIO.x_scratch (-1 for invalid dims); never part of spair_workspace_bytes */
int64_t spair_input_grad_scratch_bytes(const SpairDims* d);
/* torch.optim.Adam(lr) defaults (train.py:44) on flat buffers, one launch. */
int spair_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
               float beta1, float beta2, float eps, int step, void* stream);
/* The same update, guarded: if `skip` (device int, e.g. SpairStep.status + 1) is non-zero the whole step is left out -- parameters and
 * both moments untouched -- and counters[0] is incremented; an element whose gradient is NaN / inf is left out on its own and counters[1]
 * is set to 1.  lr * NaN never reaches a parameter.  `counters`: two device ints, caller-owned and caller-zeroed; the caller decrements its
 * bias-correction step for a skipped step if it wants torch's numbers after a recovery (FusedAdam reads the counter where it
 * synchronises anyway).  skip may be NULL (element guard only). */
int spair_adam_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                       float beta1, float beta2, float eps, int step, const int* skip, int* counters, void* stream);
/* Data-parallel replicas take ONE skip decision: exchange SpairStep.status[1] between the gradient all-reduce and the optimizer step.
 * phase 0: xchg[0..1] = bits 0 and 1 of status[1] as 0 / 1 -- all-reduce the two ints with MAX -- phase 1: status[1] = the combined bits
 * and, if any, status[0] |= them | 4 * (a bit this rank had not set itself: "flagged on another rank") and *status_host = status[0]
 * (status_host may be NULL).  `xchg`: two device ints, caller-owned.  One single-thread kernel per phase on `stream`; no synchronisation. */
int spair_status_exchange(int* status, int* xchg, int* status_host, int phase, void* stream);
/* One int of host memory that kernels can store to (hipHostMalloc, mapped + coherent), zero-initialised: SpairStep.status_host. */
int spair_host_word_alloc(int** out);
int spair_host_word_free(int* word);
/* Copy a per-row quantity of the last forward into an NCHW map [B,ch,G,Gw].
 * which: 0 z_attr, 1 z_depth, 2..7 mean of cy,cx,height,width,attr,depth, 8..13 their sigma, 14 count-prior p_z;
 * after a backward, its per-cell latent gradients: 100 d box head latents [8] (mean 4 | log-std 4), 101 d encoder output [2A], 102 d depth
 * latents [2], 103 d presence logit [1] as the per-wavefront launches store them (fp32 rows); 200..203 the same as the fused chain stores
 * them (bf16 rows) */
int spair_export_map(const SpairDims* d, const void* workspace, int which, float* out, void* stream);
/* diagnostic: stage time stamps of the fused forward chain kernel (SpairStep.flags bit 1), n <= 4096 uint64 */
int spair_chain_stamps(const SpairDims* d, const void* workspace, unsigned long long* out, int n, void* stream);
/* layout of that buffer: stamps per wavefront of the forward kernel (from offset 0; stage intervals = stamps - 1), the index of the glimpse
 * sampling interval (K4: modules.py:216-273 via models.py:387) among them, stamps per wavefront of the backward kernel (from offset 2048) */
int spair_chain_stamp_layout(int* fwd_per_wavefront, int* fwd_glimpse_interval, int* bwd_per_wavefront);
/* diagnostic: the kernels spair_forward / spair_backward choose for these dims, this workspace, SpairStep.flags `flags` and, for the
 * backward, whether an image gradient is requested (input_grad: SpairStepIO.grad_x non-NULL).  Host arithmetic only: of workspace only
 * the address's 16-byte alignment is read (it must not be NULL; nothing is dereferenced, nothing is launched).  Writes the first min(n, SPAIR_STEP_PLAN_INTS) of these ints to host `out`:
 *   [0..7]   the renderer family of the forward and of the backward (SPAIR_RENDER_*), then 0/1 for: per-object records (render_prep), fp16
 *            sprites, bf16 d-logits, the fused per-cell chain kernels, the fused decoder forward; out[7] = 0;
 *   [8..11]  0/1 for: the helper stream, the decoder's data gradients in one launch, its two small weight gradients in one grouped launch,
 *            its weight gradients issued behind the chain backward (the last three: bf16 step, MLP decoder);
 *   [12]     the first backbone layer of the fused trailing 1x1 stack (layer 0 is the stem, conv_out is layer n_conv; n_conv + 1: none);
 *   [13]     where the stem's weight gradient is taken (SPAIR_STEM_*);
 *   [14..21] per backbone layer 1 .. 8 (conv_out included) the forward kernel (SPAIR_CONV_*), -1 past conv_out;
 *   [22..29] the same for its data gradient;
 *   [30..37] 0/1: the layer's data gradient reads its ReLU gate as the sign bits the forward of the layer below left (else the stored
 *            activation), -1 past conv_out. */
#define SPAIR_STEP_PLAN_INTS 38
#define SPAIR_RENDER_MMA 0      /* matrix-core forward on records (render3.hip) */
#define SPAIR_RENDER_GEN2 1     /* k_render_fwd3 / k_render_bwd2 (render2.hip) */
#define SPAIR_RENDER_GEN1 2     /* k_render_fwd / k_render_bwd (render.hip) */
#define SPAIR_RENDER_COLOUR 3   /* C = 2 or 3 channels (render_c.hip) */
#define SPAIR_CONV_GEMM 0       /* one implicit-GEMM launch in the step's dtype (a strided data gradient: all output-parity classes in it) */
#define SPAIR_CONV_PATCH 1      /* the patch-resident kernel of 128 -> 128 channel 4x4 / stride-2 layers (conv_s2.hip, conv_s2_dgrad.hip) */
#define SPAIR_CONV_PER_CLASS 2  /* one implicit-GEMM launch per output-parity class */
#define SPAIR_CONV_PW_STACK 3   /* the fused trailing stack of 1x1 layers (pointwise.hip) */
#define SPAIR_STEM_PATCH 0      /* fused into conv_1's patch-resident data gradient */
#define SPAIR_STEM_GEMM 1       /* fused into the epilogue of conv_1's implicit-GEMM data gradient */
#define SPAIR_STEM_WGRAD16 2    /* its own kernel (grey-scale 4x4 stem, bf16 step) */
#define SPAIR_STEM_GENERIC 3    /* the TN GEMM (fp32 step, other stems) */
int spair_step_plan(const SpairDims* d, const void* workspace, int flags, int input_grad, int* out, int n);
/* diagnostic: where the buffer `name` of a step's workspace lies, for the step plan of (flags, input_grad) as spair_step_plan takes them.
 * Host arithmetic only, as spair_step_plan (workspace is an address, never dereferenced).  Writes to host `out`: [0] byte offset from
 * workspace, [1] rows, [2] meaningful columns, [3] leading dimension in elements, [4] element type (0 fp32, 1 bf16, 2 fp16) as that plan
 * writes the buffer, [5] 1 if that plan's training step (forward + backward) writes it, else 0.  No buffer is aliased: the regions never
 * overlap, and every one keeps what the last step left until the next step on the workspace.  Returns SPAIR_ERR_SHAPE for an unknown name,
 * SPAIR_ERR_UNSUPPORTED for a buffer these dims do not allocate.  Names (rows r = cprime * B + b in dependency-wavefront order, N = B Gh Gw):
 *   per-cell rows, N each -- bf16 from the fused chain, fp32 from the per-wavefront launches (SpairStep.flags bit 0), except the head outputs
 *   Ob, Oe, Oz, Oo (fp32 always) and dGl (fp32):
 *     Xb [features | context], Hb1, Hb2 (box network hidden), Ob [pass NP | lat 8]; glimpse, He1, He2, Oe [mean A | logstd A] (encoder);
 *     Xz [features | context | pass | box 4 | attr A], Hz1, Hz2, Oz [pass NP | lat 2]; Xo [Xz's columns | depth], Ho1, Ho2, Oo [logit];
 *     dXb dHb1 dHb2 dOb dGl dHe1 dHe2 dOe dXz dHz1 dHz2 dOz dXo dHo1 dHo2 dOo: their gradients (the fused chain stores no dXb / dXz / dXo,
 *     and dGl only for an image gradient; its first layers read Xb's [features | context] columns in place of Xz's / Xo's);
 *     Za, Za16: the decoder's input (z_attr; fp32 from the per-wavefront launches, its bf16 copy in the bf16 step)
 *   decoder: Hd1, Hd2, dHd1, dHd2 (hidden layers and their gradients, the step's dtype), S (sprite logits / sprites: fp16 or fp32 as
 *     spair_step_plan's s16), dLog (d logits: bf16 or fp32 as its g16), dLog16 (bf16 copy of fp32 d logits, bf16 step)
 *   backbone (NHWC, one row per pixel): xpad (padded input, fp32), act<i> / dact<i> (output of layer i = 0 .. n_conv - 1 and its gradient, the
 *     step's dtype; dact0 is not written where conv_1's data gradient takes the stem's weight gradient), feat / dfeat (conv_out's output
 *     and its gradient, fp32, N rows; dfeat is not written by the fused chain), dfeat16 (bf16 copy of dfeat, bf16 step)
 *   prepared weights (the step's dtype, zero padded to the leading dimension): conv_wf<i> (layer i = 1 .. n_conv: [cout][k k cin], taps
 *     (ky, kx) outer, or the tap-parity K order of the bf16 strided convs with cin % 64 == 0), conv_wd<i>_<q> (its data-gradient matrix of
 *     output-parity class q = py s + px: [cin][(ty T + tx) cout + co] of W[co][ci][py + s ty][px + s tx], T = k / s; 1x1: [cin][cout]),
 *     lin_wf.<layer> ([out][in]) and lin_wt.<layer> ([in][out]) per dense layer, named as its parameters without ".weight" (the two
 *     output layers of a head share one matrix: output_layers.0 sits behind output_layers.1's rows / columns). */
int spair_workspace_view(const SpairDims* d, const void* workspace, int flags, int input_grad, const char* name, long long* out);
/* the idx-th name spair_workspace_view resolves on these dims (the buffers they allocate), or SPAIR_ERR_SHAPE past the last one */
int spair_workspace_view_name(const SpairDims* d, int idx, char* name, int name_cap);
/* wavefronts walked by the workgroup that stamps (sample 0; with the band split of grids wider than 16 cells, its top band) */
int spair_chain_stamp_wavefronts(const SpairDims* d);
/* band split of the fused per-cell kernels (grids wider than 16 cells: ceil(G / 8) workgroups per sample hand the boundary rows' records /
 * context gradients to each other through `workspace`): writes 1 to *out (device int) if a bounded wait EVER timed out in a
 * spair_forward / spair_backward on this workspace (sticky: only re-zeroing the workspace clears it; from that step on loss_out[0] and the
 * gradient of virtual_edge_element are NaN, so a training loop sees it without calling this), 0 if not, -1 where the kernels run unsplit */
int spair_chain_sync_status(const SpairDims* d, const void* workspace, int* out, void* stream);
/* the four noise maps [B,{4,A,1,1},G,Gw] of one step from a Philox stream */
int spair_noise_fill(const SpairDims* d, uint64_t seed, float* eps_box, float* eps_attr, float* eps_depth, float* u_pres, void* stream);

/* Opt-in instrumentation for bench.py: HIP events on the caller's stream around regions of the step.
 * slots: 0 prep, 1 backbone fwd, 2 per-cell chain fwd, 3 decoder fwd, 4 count-prior KL, 5 render fwd (1 kernel),
 * 6 KL+loss, 7 render bwd (1 kernel), 8 decoder bwd, 9 per-cell chain bwd, 10 per-cell weight grads,
 * 11 backbone bwd, 12 conv_1 fwd (1 kernel), 13 decoder.out fwd GEMM (1 kernel), 14 STN glimpse fwd (per wavefront),
 * 15 adam, 16 decoder.out wgrad, 17 decoder.out dgrad.  spair_prof_read synchronises: call it outside timed regions. */
int spair_prof_enable(int enable);                      /* 0 stop, 1 start afresh, 2 resume (keeps earlier records) */
int spair_prof_select(unsigned long long slot_mask);   /* record only the regions whose bit is set (default: all) */
int spair_prof_read(float* ms, int* counts, int nslots);

/* ---- unit-level entry points (each kernel can be parity-checked alone) --------------------- */
int spair_gemm_nt(const float* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K,
                  const float* bias, const float* relu_mask, int ldmask, int relu, int accumulate, int dtype,
                  void* stream);
int spair_gemm_tn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int R,
                  int dtype, void* stream);
int spair_gemm_nt_conv(const float* In, const int* conv13, const void* B, int ldb, float* C, int ldc, int M,
                       int N, int K, const float* bias, const float* relu_mask, int ldmask, int relu,
                       int accumulate, const int* cmap8, int dtype, void* stream);
int spair_gemm_tn_conv(const float* A, int lda, const float* In, const int* conv13, float* C, int ldc, int M,
                       int N, int R, int dtype, void* stream);
int spair_colsum(const float* A, int lda, int R, int N, float* out, void* stream);
/* Direct fp32 convolutions of the convolutional object encoder / decoder variant (objconv.hip; SpairDims.obj_conv).  A tensor is
 * described by t6 = {rs, ys, xs, cs, H, C}: element (r, y, x, c) at p[r*rs + y*ys + x*xs + c*cs], H x H pixels, C channels.  W is
 * [X][Y][k][k] (nn.Conv2d: X = out, Y = in channels; nn.ConvTranspose2d: X = in, Y = out channels).
 * spair_objconv_gather, transposed = 0: out(r,y,x,X) = bias + sum in(r, y*s+ky, x*s+kx, Y) * W  (Conv2d forward / ConvTranspose2d data
 *   gradient); transposed = 1: out(r,y,x,Y) = bias + sum in(r, (y-ky)/s, (x-kx)/s, X) * W  (ConvTranspose2d forward / Conv2d data
 *   gradient); then out = 0 where gate <= 0 (gate: same layout as out, or NULL), then ReLU if relu.
 * spair_objconv_wgrad: G[cs][cb][ky][kx] += sum small(r,y,x,cs) * big(r, y*s+ky, x*s+kx, cb), bias_small[cs] += sum small (or NULL)
 *   (Conv2d: small = d out, big = in; ConvTranspose2d: small = in, big = d out). */
int spair_objconv_gather(int transposed, const float* in, const long long* in6, const float* W, const float* bias, float* out,
                         const long long* out6, const float* gate, int k, int s, int relu, long long R, void* stream);
int spair_objconv_wgrad(const float* small, const long long* small6, const float* big, const long long* big6, float* G,
                        float* bias_small, int k, int s, long long R, void* stream);
/* bf16-STORED operand GEMMs (the bf16 mode's activations and gradients live in HBM as bf16; same roles as above).
 * spair_gemm_nt16: C = epi(A * B^T), A bf16 [M][lda] or an NHWC conv gather (conv13), B bf16 [N][ldb], C bf16 (c_bf16)
 *   or fp32; relu_mask bf16 (mask_bf16) or fp32; cmap8 remaps output rows (stride-2 conv data gradient by parity class).
 * spair_gemm_tn16: C += A^T * B over R rows, A bf16 [R][lda], B bf16 rows / bf16 or fp32 conv gather; cw_cin/cw_taps store
 *   columns in OIHW order; colsum_out += column sums of A (bias gradient).  scratch (optional, >= blocks*128*128 floats):
 *   split-K partial tiles + a reduce pass instead of fp32 atomics (modules.py:59-64,124-165 autograd). */
int spair_gemm_nt16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                    const float* bias, const void* relu_mask, int ldmask, int mask_bf16, int relu, int c_bf16,
                    const int* conv13, const int* cmap8, void* stream);
int spair_gemm_tn16(const void* A, int lda, const void* B, int ldb, int b_bf16, float* C, int ldc, int M, int N,
                    int R, const int* conv13, int cw_cin, int cw_taps, float* colsum_out, float* scratch,
                    long long scratch_floats, void* stream);
/* weight + bias gradient of the single-channel 4x4 stem conv with 128 filters (Backbone layer 0, modules.py:59-64):
 * dY bf16 [B*Hout*Hout][128], xpad fp32 [B][Hin][Hin]; dW [128][1][4][4] and db [128] are accumulated;
 * scratch >= 512*128*32 floats */
int spair_stem_wgrad16(const void* dY, const float* xpad, float* dW, float* db, float* scratch,
                       long long scratch_floats, int B, int Hin, int stride, int Hout, void* stream);
/* Fused stack of L <= 4 1x1 convolutions on bf16 NHWC activations with 128 channels (Backbone's trailing 1x1 layers + conv_out,
 * modules.py:59-64,107-111).  Host arrays of L device pointers.
 * fwd: Y_l = relu(Y_{l-1} W_l^T + b_l); W[l] bf16 [cout_l][ldw_l]; Y[l] bf16 [M][128] for l < L-1; the last layer has no relu and
 *      writes fp32 Ylast [M][ldlast] (cout_{L-1} <= 128 columns).
 * bwd: layers in BACKWARD order; dX_l = (dX_{l-1} Wd_l^T) * [gate_l > 0]; dY bf16 [M][ldd] (kd valid columns), Wd[l] bf16
 *      [128][ldw_l] = W transposed, gate[l] = the layer's forward INPUT (bf16 [M][128]), dX[l] bf16 [M][128]. */
int spair_conv1x1_stack_fwd16(const void* X, const void* const* W, const int* ldw, const int* cout,
                              const float* const* bias, void* const* Y, float* Ylast, int ldlast, int M, int L,
                              void* stream);
int spair_conv1x1_stack_bwd16(const void* dY, int ldd, int kd, const void* const* Wd, const int* ldw, const int* cout,
                              const void* const* gate, void* const* dX, int M, int L, void* stream);
/* ---- evaluation metrics (spair/metric.py:5-99), device-side, no in-place mutation ------------------------------ */
/* z_where [B,4,G,G] (x, y, w, h image fractions, the reference's top-left convention), z_pres [B,1,G,G], bbox [B,K,4]
 * (x, y, w, h px, zero padded), count [B] fp32; scratch 2*B floats; out[0] = mAP (metric.py:5-47),
 * out[1] = object_count_accuracy (metric.py:49-56) */
int spair_metrics(const float* z_where, const float* z_pres, const float* bbox, const float* count, int B, int G,
                  int image_side, int K, float* scratch, float* out, void* stream);
/* batch_jaccard (metric.py:82-99): corner-format boxes [B,A,4] x [B,Bn,4] -> iou [B,A,Bn] */
int spair_batch_jaccard(const float* box_a, const float* box_b, int B, int A, int Bn, float* iou, void* stream);
/* ---- synthetic scattered-digit scenes generated on the device (stands in for spair/dataloader.py:10-36, whose HDF5 file is not
 * available; same item contract).  image [B,1,I,I] fp32 in [0,1], bbox [B,K,4] fp32 (x, y, w, h px, zero padded), count [B] int64;
 * samples first..first+B-1 of the Philox stream `seed`; scratch B*K*28 floats. */
int spair_scenes_generate(uint64_t seed, long long first, int B, int I, int K, int size_min, int size_max, float* image,
                          float* bbox, long long* count, float* scratch, void* stream);
/* fp32 [rows][ld_src] -> bf16 [rows][ld_dst] (round to nearest even), first `cols` columns */
int spair_cast_bf16(const float* src, int ld_src, void* dst, int ld_dst, long long rows, int cols, void* stream);
/* stn(image, z_where, [P,P]) forward (border) and its gradient wrt z_where (modules.py:216-273);
 * row r samples image x[r % B], nbox[r] = (xt,yt,xs,ys) */
int spair_stn_glimpse_fwd(const float* x, const float* nbox, int B, float* glimpse, int ld_gl, int R, int C,
                          int I, int P, int align_corners, void* stream);
int spair_stn_glimpse_bwd(const float* x, const float* nbox, int B, const float* dglimpse, int ld_gl,
                          float* dnbox, int R, int C, int I, int P, int align_corners, void* stream);
/* The two kernels of the step's image gradient (SpairStepIO.grad_x) on their own (csrc/input_grad.hip).
 * spair_input_grad_glimpse: adjoint of spair_stn_glimpse_fwd with respect to the IMAGE.  Rows r = k*B + b (k < ncell) of dglimpse
 * [rows][ld_gl] ((c, i, j) order) and nbox [rows][4]; out [B,C,I,I] = sum over k of sample b's rows, overwritten, deterministic.
 * spair_input_grad_stem: data gradient of the stem conv (weights w [Cout,C,k,k], stride s) from dact0 [B,Hout,Hout,Cout] (fp32, or bf16 with
 * dact_bf16), cropped by pad_pre to grad_x [B,C,I,I] (overwritten) and plus add [B,C,I,I] (NULL = none). */
int spair_input_grad_glimpse(const float* nbox, int B, int ncell, const float* dglimpse, int ld_gl, float* out, int C, int I, int P,
                             int align_corners, void* stream);
int spair_input_grad_stem(const void* dact0, int dact_bf16, const float* w, int B, int C, int I, int pad_pre, int k, int s, int Hout,
                          int Cout, const float* add, float* grad_x, void* stream);
/* stn(sprites, z_where, [I,I], inverse=True) materialised (modules.py:256-269): sprites [N,C,P,P] -> out [N,C,I,I], bilinear, zeros
 * padding, inverse affine in closed form; backward ACCUMULATES into dsprites [N,C,P,P] and dnbox [N,4] (zero them first).  Only for
 * callers of the reference's helper -- the training step never materialises this tensor (spair_render_fwd fuses it). */
int spair_stn_inverse_fwd(const float* sprites, const float* nbox, float* out, int N, int C, int P, int I, int align_corners,
                          void* stream);
int spair_stn_inverse_bwd(const float* sprites, const float* nbox, const float* grad_out, float* dsprites, float* dnbox, int N,
                          int C, int P, int I, int align_corners, void* stream);
/* renderer: inverse STN + importance-weighted composite + BCE (models.py:485-547) */
int spair_render_fwd(const float* sprites, int ld_s, const float* nbox, const float* pres, const float* depth,
                     const float* x, float* recon, float* aux /* B*I*I float2: (dBCE/dpre / D, pre) */, float* bce_partial,
                     int B, int HW, int C, int I, int P, int align_corners, void* stream);
int spair_render_bwd(const float* sprites, int ld_s, const float* nbox, const float* pres, const float* depth,
                     const float* aux, const float* grad_loss, float* dlogits, float* dnbox, float* dpres, float* ddepth,
                     int B, int HW, int C, int I, int P, int align_corners, float obj_scale, float alpha_scale, void* stream);
/* The same for images with C = 2 or 3 colour channels (cfg.INPUT_IMAGE_SHAPE[0], models.py:480,524; render_c.hip): sprites fp32
 * [N][ld_s] = [P*P][C+1] (colour.., alpha) after the sigmoid, x / recon [B][C][I][I], aux B*C*I*I float2, dlogits fp32 [N][ld_s].
 * Generic-channel kernels (correctness and run-to-run determinism; the tuned renderers are single-channel). */
int spair_render_fwd_rgb(const float* sprites, int ld_s, const float* nbox, const float* pres, const float* depth, const float* x,
                         float* recon, float* aux, float* bce_partial, int B, int HW, int C, int I, int P, int align_corners, void* stream);
int spair_render_bwd_rgb(const float* sprites, int ld_s, const float* nbox, const float* pres, const float* depth, const float* aux,
                         const float* grad_loss, float* dlogits, float* dnbox, float* dpres, float* ddepth, int B, int HW, int C, int I,
                         int P, int align_corners, float obj_scale, float alpha_scale, void* stream);
/* Backbone stem alone: conv 1 -> Cout channels, 4x4, stride `stride`, no padding, + bias + relu, over the image zero-padded to Hin x Hin
 * (pad_pre pixels before; modules.py:95-104 Backbone.padding + the first Conv2d/ReLU of Backbone.net).  x [B][I][I] fp32 (unpadded),
 * w [Cout][16], out NHWC [B][Hout][Hout][Cout] fp32 or (out_bf16) bf16.  In bf16 mode with Cout = 128, stride 2 it runs on the matrix
 * cores with split-bf16 operands (three products, fp32 accumulation): agrees with the fp32 result to < 2^-15 relative before the store. */
int spair_stem_conv_fwd(const float* x, const float* w, const float* bias, void* out, int B, int I, int pad_pre, int Hin, int Hout,
                        int Cout, int stride, int out_bf16, void* stream);
/* Patch-resident forward of the backbone's 128 -> 128 channel, 4x4, stride-2 convolutions + bias + ReLU (reference modules.py:59-64), bf16 NHWC in / out
 * (csrc/conv_s2.hip).  in16 [B][Hin][Hin][128] with Hin = 2 * Hout + 2 (the input is pre-padded); wf16 [128][2048] bf16 in tap-parity K order:
 * column ((class * 2 + half) * 4 + tap) * 64 + c holds W[o][ci = half * 64 + c][ky = py + 2 dy][kx = px + 2 dx], class = 2 py + px, tap = 2 dy + dx;
 * out16 [B * Hout * Hout][128].  Returns SPAIR_ERR_UNSUPPORTED when a 256-row tile's input patch exceeds the kernel's LDS buffer. */
int spair_conv_s2k4_fwd16(const void* in16, const void* wf16, const float* bias, void* out16, int B, int Hin, int Hout, void* stream);
/* The same launch leaving, beside its output, the sign-bit mask described below (mask8 [B * Hout * Hout][16] bytes, bit e of byte g =
 * channel 8 g + e of the stored bf16 output > 0): what the training step runs where the next layer's data gradient reads its gate as bits.
 * The output is bit-identical to spair_conv_s2k4_fwd16's.  SPAIR_ERR_SHAPE for a NULL mask8. */
int spair_conv_s2k4_fwd16_mask(const void* in16, const void* wf16, const float* bias, void* out16, void* mask8, int B, int Hin, int Hout,
                               void* stream);
/* The tiling the two patch-resident launchers choose -- the very code they run, host arithmetic only (no device is needed, nothing is
 * launched).  dgrad = 0: spair_conv_s2k4_fwd16 with H = Hout (tiles of 256 output pixels); dgrad = 1: spair_conv_s2k4_dgrad16 / _bits with
 * H = Ho (tiles of 128 pixels of one output-parity class grid, (Ho + 1)^2 per image; the launch is persistent, min(tiles, CUs) workgroups).
 * Writes *tiles and *tpi (tiles per image when every tile restarts at an image, 0 when the tiles run over the whole batch) and returns
 * SPAIR_OK, or SPAIR_ERR_UNSUPPORTED where the launcher refuses the shape. */
int spair_conv_s2k4_tiling(int dgrad, int B, int H, int* tiles, int* tpi);
/* Patch-resident DATA GRADIENT of the same layers (csrc/conv_s2_dgrad.hip): dout16 bf16 NHWC [B][Ho][Ho][128]; wdq: bf16 [128 ci][4 * 128], column
 * (ty * 2 + tx) * 128 + co = W[co][ci][py + 2 ty][px + 2 tx] for output-parity class q = 2 py + px; gate16: the stored activation of the layer
 * below, bf16 NHWC [B][2 (Ho + 1)][2 (Ho + 1)][128]; out16 (same shape) = conv2d_backward_input(dout, W) where gate16 > 0, else 0. */
int spair_conv_s2k4_dgrad16(const void* dout16, const void* wd0, const void* wd1, const void* wd2, const void* wd3, const void* gate16,
                            void* out16, int B, int Ho, void* stream);
/* Sign-bit form of a ReLU gate (round 5): one byte per (pixel, 8 channels), [B][H][H][16], bit e = channel 8 g + e of the stored bf16
 * activation > 0.  spair_stem_conv_fwd_mask: the stem (1 -> 128 channels, 4 x 4, stride 2, bf16 output) leaving that mask beside its output;
 * spair_conv_s2k4_dgrad16_bits: spair_conv_s2k4_dgrad16 reading the gate from it (20 MB instead of the 321-MB activation at the benchmark
 * shape) -- what the training step runs for conv_1's data gradient. */
int spair_stem_conv_fwd_mask(const float* x, const float* w, const float* bias, void* out, void* mask8, int B, int I, int pad_pre, int Hin,
                             int Hout, void* stream);
int spair_conv_s2k4_dgrad16_bits(const void* dout16, const void* wd0, const void* wd1, const void* wd2, const void* wd3,
                                 const void* gate_bits8, void* out16, int B, int Ho, void* stream);
/* The bf16 step's object-decoder FORWARD (reference models.py:474-492: Linear 50->128, ReLU, Linear 128->256, ReLU, Linear 256->P*P*2, the sprite
 * scales and analytic sigmoid) as one activation-stationary kernel (csrc/dec_fused.hip).  z_attr16: bf16 [N][ld_za] (columns >= A ignored);
 * W*, b*: the fp32 parameters, row-major [out][in]; H1 / H2: bf16 [N][128] / [N][256] hidden activations (stored for the backward);
 * sprites: fp16 [N][ld_s] (grey, alpha) pairs; stream_buf: spair_decoder_fwd16_scratch_bytes(n_out) bytes of scratch (the packed weights). */
int64_t spair_decoder_fwd16_scratch_bytes(int n_out);
int spair_decoder_fwd16(const void* z_attr16, int ld_za, const float* W0, const float* b0, const float* W1, const float* b1,
                        const float* W2, const float* b2, void* H1, void* H2, void* sprites, int ld_s, long long N, int A, int n_out,
                        float obj_scale, float alpha_scale, float alpha_bias, void* stream_buf, void* stream);
/* The decoder's DATA-GRADIENT chain (autograd of the three Linear layers of models.py:474-484 w.r.t. their inputs; csrc/dec_fused_bwd.hip) in one
 * launch.  dlogits16: bf16 [N][ld_s] (n_out columns, the sigmoid's derivative already applied); W2t16 / W1t16 / W0t16: the TRANSPOSED weights as
 * bf16, [256][ld2], [128][256], [A][128]; H2 / H1: the stored forward activations bf16 [N][256] / [N][128] (relu gates); outputs: dH2 / dH1 (bf16,
 * same shapes) and d_z_attr fp32 [N][ld_dza] (A columns written).  A <= 64, n_out % 8 == 0. */
int spair_decoder_bwd16(const void* dlogits16, int ld_s, const void* W2t16, int ld2, const void* W1t16, const void* W0t16, const void* H2,
                        const void* H1, void* dH2, void* dH1, float* d_z_attr, int ld_dza, long long N, int A, int n_out, void* stream);
/* the same with 16-bit sprites, as the bf16 training step runs them: sprites are FP16 (grey, alpha) pairs [N][ld_s] (post-sigmoid values
 * in (0,1): 11 significant bits), d-logits come back as BF16 [N][ld_s] */
int spair_render_fwd16(const void* sprites_f16, int ld_s, const float* nbox, const float* pres, const float* depth,
                       const float* x, float* recon, float* aux, float* bce_partial, int B, int HW, int C, int I, int P,
                       int align_corners, void* stream);
int spair_render_bwd16(const void* sprites_f16, int ld_s, const float* nbox, const float* pres, const float* depth,
                       const float* aux, const float* grad_loss, void* dlogits_bf16, float* dnbox, float* dpres, float* ddepth,
                       int B, int HW, int C, int I, int P, int align_corners, float obj_scale, float alpha_scale, void* stream);
/* The forward renderer of the bf16 step on the matrix cores (csrc/render3.hip; same reference lines: stn(inverse=True) modules.py:256-269 +
 * the composite models.py:511-540).  The inverse-STN sampling is separable, out_c = Wy . S_c . Wx^T with hat weights, and runs as three
 * v_mfma_f32_16x16x32_f16 per channel and (object, 16 x 16 tile) on the fp16 sprites as they lie in memory.
 * spair_render_prep writes 64 bytes of records per object (source-coordinate coefficients, presence, importance scale / floor, pixel footprint,
 * raw inverse-affine parameters; sample-major, 64 * B * HW bytes, 16-byte aligned, caller-owned) from the rows r = k * B + b of nbox [N][4] / pres [N] / depth [N];
 * spair_render_fwd16m composites from the records: same outputs as spair_render_fwd16 (recon, aux, bce_partial), per pixel within 5e-4 of
 * it (fp16 hat weights on source coordinates rounded to 2^-11 texel, one fp16 rounding of the x-interpolated rows), unbiased.
 * SPAIR_ERR_UNSUPPORTED for P != 28, align_corners, HW > 1024: use spair_render_fwd16. */
int spair_render_prep(const float* nbox, const float* pres, const float* depth, void* records, int B, int HW, int I, int P,
                      int align_corners, void* stream);
int spair_render_fwd16m(const void* sprites_f16, int ld_s, const void* records, const float* x, float* recon, float* aux,
                        float* bce_partial, int B, int HW, int C, int I, int P, int align_corners, void* stream);
/* spair_render_bwd16 with the inverse-affine parameters and pixel footprints read from the records of spair_render_prep (the same nbox /
 * pres / depth) instead of recomputed per object: what the training step runs; identical outputs */
int spair_render_bwd16r(const void* sprites_f16, int ld_s, const float* nbox, const float* pres, const float* depth, const void* records,
                        const float* aux, const float* grad_loss, void* dlogits_bf16, float* dnbox, float* dpres, float* ddepth,
                        int B, int HW, int C, int I, int P, int align_corners, float obj_scale, float alpha_scale, void* stream);
/* ---- scene parse: the renderer's per-pixel assignment (csrc/render_owner.hip; the reference's composite, models.py:524-537, kept per
 * object instead of summed).  For sample b, pixel (y, x) of the I x Iw canvas and cell k = h * Gw + w (ROW-MAJOR grid order), with the
 * renderer's bilinear, zero-padded inverse-STN sampling:
 *     a_k = warp(alpha_k * pres_k),  m_k = warp(max(alpha_k * pres_k * depth_k, 0.01)),  D = sum_k m_k + HW * 1e-9,
 *     w_k = a_k (m_k + 1e-9) / D   (the coefficient of object k's colour in the composite),
 *     coverage = sum_k w_k,  owner_weight = max_k w_k (always the raw maximum),
 *     owner = the smallest k with w_k = owner_weight if that is > 0 and >= threshold, else -1,  area[b][k] = pixels of sample b with owner k.
 * Outputs: owner int32 [B][I][Iw], owner_weight / coverage fp32 [B][I][Iw], area int32 [B][HW] (zeroed by the call; integer atomics).  No
 * float atomics: bit-identical from run to run.  HW <= 1024.
 * spair_render_owner (unit level): sprites [N][ld_s] of fp16 (s16 = 1) or fp32 elements, P*P texels of `ch` elements each with alpha (after
 *   the sigmoid) LAST -- ch = 2: the grey (grey, alpha) pairs, ch = C + 1: the colour sprites; nbox [N][4], pres [N], depth [N]; cell k of
 *   sample b is row r = (cidx ? cidx[k] : k) * B + b, cidx: HW device ints or NULL.
 * spair_parse_owner (step level): the same on the sprites and the nbox / presence / depth rows the latest spair_forward left in
 *   `workspace`, in the formats spair_step_plan(flags) says it wrote, through the workspace's own cell-to-row table. */
int spair_render_owner(const void* sprites, int ld_s, int s16, int ch, const float* nbox, const float* pres, const float* depth,
                       const int* cidx, float threshold, int* owner, float* owner_weight, float* coverage, int* area, int B, int HW, int I,
                       int Iw, int P, int align_corners, void* stream);
int spair_parse_owner(const SpairDims* d, const void* workspace, int flags, float threshold, int* owner, float* owner_weight,
                      float* coverage, int* area, void* stream);
/* The cell-to-row table of a workspace (written by the first spair_forward on it): out[k] = cprime of cell k = h * Gw + w, G * Gw device
 * ints; the per-cell rows of spair_workspace_view are r = cprime * B + b. */
int spair_cell_rows(const SpairDims* d, const void* workspace, int* out, void* stream);
/* ---- scene composition: a scene rendered from GIVEN latents (csrc/compose.hip; the reference's _render, models.py:452-542, is a pure
 * function of them), and its composite kept per requested object.
 * spair_compose: z_where [B][4][G][Gw] = (xt, yt, xs, ys), z_what [B][A][G][Gw], z_depth / z_pres [B][1][G][Gw] (device, fp32, taken as
 *   given: nothing is clamped) -> recon [B][C][I][Iw] and, where inv_den is not NULL, the composite's 1/D per pixel [B][I][Iw].  It runs the
 *   cell tables, the object decoder's share of the weight preparation from `params`, the latents into the workspace's per-cell rows (the
 *   inverse of spair_export_map 0 / 1; nbox = z_where), then the decoder and the renderer forward that spair_step_plan(flags) names -- what
 *   spair_forward runs after its per-cell chain.  No backbone, no chain, no KL, no loss: SpairStep.status is not written.  It overwrites
 *   the workspace's decoder / renderer buffers as any forward does (a spair_backward of an earlier forward on it is then meaningless).
 * spair_render_layers: on the sprites and rows the latest spair_compose / spair_forward left in `workspace`, for cells [B][K] (device
 *   ints, row-major cell index k = h * Gw + w; any value outside [0, G * Gw): an all-zero layer; duplicates allowed) and that call's inv_den:
 *     layer_weight[b][j] = a_k (m_k + 1e-9) / D  (the w_k of the scene parse above),  layers[b][j][c] = layer_weight[b][j] * warp(colour_k[c]),
 *   layers [B][K][C][I][Iw], layer_weight [B][K][I][Iw], every element written (zeros outside a footprint).  The sum of the layers of ALL
 *   cells is recon before its clamp.  No atomics: bit-identical from run to run.
 * spair_render_layers_rows (unit level): the same on explicit operands, laid out as for spair_render_owner; ch = 2 .. 4. */
int spair_compose(const SpairDims* d, const float* params, void* workspace, int flags, const float* z_where, const float* z_what,
                  const float* z_depth, const float* z_pres, float* recon, float* inv_den, void* stream);
int spair_render_layers(const SpairDims* d, const void* workspace, int flags, const int* cells, int K, const float* inv_den, float* layers,
                        float* layer_weight, void* stream);
int spair_render_layers_rows(const void* sprites, int ld_s, int s16, int ch, const float* nbox, const float* pres, const float* depth,
                             const int* cidx, const int* cells, int K, const float* inv_den, float* layers, float* layer_weight, int B,
                             int HW, int I, int Iw, int P, int align_corners, void* stream);
/* ---- scene generation: latents drawn from the model's own prior (csrc/prior.hip; the generative process the loss assumes, reference
 * models.py:169-262).  Cells in row-major order i = h * Gw + w, HW = G * Gw <= 1024.
 * spair_prior_presence (unit level, no model): u [B][HW] uniform draws in [0, 1) -> z_pres [B][HW] (hard: 0.0 or 1.0), p_z [B][HW],
 *   n_present int32 [B] = the sum of z_pres.  With cd the distribution of the object count c = 0 .. HW, started from
 *   normalise((1 - count_prior_prob) count_prior_prob^c), `seen` the objects so far and rem = HW - i:
 *       q_c = clamp(c - seen, 0, rem) / rem,  p_z(i) = sum_c cd_c q_c,  z_i = [u_i < p_z(i)],
 *       cd <- cd (z_i q + (1 - z_i)(1 - q)) / max(its sum, 1e-6),  seen += z_i.
 *   count != NULL (B device ints): sample b holds exactly n = clamp(count[b], 0, HW) objects, uniformly placed -- the same recursion from
 *   the one-hot distribution at n, in closed form: p_z(i) = fl32((n - seen) / rem), correctly rounded (exactly 1 when n - seen == rem,
 *   exactly 0 when n == seen); count_prior_prob is then not read.  One wave per sample, no atomics: bit-identical from run to run.
 *   SPAIR_ERR_SHAPE before any launch for B < 1, HW < 1 or > 1024, a NULL u / z_pres / p_z / n_present, and, with count == NULL, a
 *   count_prior_prob that is not strictly inside (0, 1) (NaN included).
 * spair_prior_sample: the four noise maps of a step (eps_box [B][4][G][Gw], eps_attr [B][A][G][Gw], eps_depth / u_pres [B][1][G][Gw]) ->
 *   z_where [B][4][G][Gw] = (xt, yt, xs, ys), z_what [B][A][G][Gw], z_depth [B][1][G][Gw] and z_pres / p_z [B][1][G][Gw], n_present [B] as
 *   above.  The raw latent is prior_mean + prior_std * eps (SpairDims order cy, cx, height, width, attr, depth), then the step's own box
 *   and depth transforms; z_what is the raw latent.  Reads no parameters, no workspace, no SpairStep.status; both kernels on `stream`.
 *   What spair_compose takes. */
int spair_prior_presence(const float* u, int B, int HW, float count_prior_prob, const int* count /* [B] or NULL */,
                         float* z_pres, float* p_z, int* n_present, void* stream);
int spair_prior_sample(const SpairDims* d, float count_prior_prob, const int* count,
                       const float* eps_box, const float* eps_attr, const float* eps_depth, const float* u_pres,
                       float* z_where, float* z_what, float* z_depth, float* z_pres, float* p_z, int* n_present, void* stream);
/* ---- evaluation: the loss of one forward per image, per cell and per pixel (csrc/evaluate.hip; reference models.py:169-262, 544-563).
 * Cells in row-major order k = h * Gw + w, HW = G * Gw <= 1024; row r = (cidx ? cidx[k] : k) * B + b; element (r, col) of a per-row
 * array p with leading dimension ld is p[r * ld + col].
 *   kl_map [B][7][HW]: j = 0 .. 5 (cy, cx, height, width, attr, depth): z_pres 0.5 (vr + t1 - 1 - log vr), vr = (sd / s)^2,
 *       t1 = ((mu - m) / s)^2 against the prior (m, s) of that latent, attr summed over its A elements;
 *       j = 6: z (log(z + 1e-9) - log(p_z + 1e-9)) + (1 - z)(log(1 - z + 1e-9) - log(1 - p_z + 1e-9)) on the STORED p_z.
 *   bce_map [B][I][Iw]: sum over the C channels of -(x max(log recon, -100) + (1 - x) max(log(1 - recon), -100))   (torch's clamp).
 *   terms [B][9]: 0: bce + beta * (sum of 2 .. 8), 1: bce, 2 .. 8: the seven KLs of the sample -- nats per image, unscaled: the batch
 *       scalars of spair_forward's loss_out are loss_out[1] = sum_b terms[b][1], loss_out[2 + j] = kl_scale * sum_b terms[b][2 + j].
 * kl_map / bce_map may be NULL (not computed); on them map = (accumulate ? map : 0) + scale * value (one writer per element: K calls
 * with scale = 1 / K, the first with accumulate = 0, leave the mean over K draws); terms is always written plainly.
 * scratch: spair_sample_terms_scratch_floats(B, HW, I, Iw) floats (device), the per-workgroup partial sums; its size and the order of
 * every sum depend on the shape alone.  No atomics: bit-identical from run to run.  Two launches on `stream`.
 * spair_sample_terms_rows (unit level, no model, no workspace): the caller's arrays -- z_pres, p_z, mu_depth, sd_depth: one column;
 *   mu_box / sd_box: four columns (cy, cx, height, width); mu_attr / sd_attr: A columns; cidx: HW device ints or NULL (identity);
 *   prior_mean / prior_std: six HOST floats (cy, cx, height, width, attr, depth); recon, x [B][C][I][Iw].
 * spair_eval_terms: the same on what the latest spair_forward left in `workspace` (its rows' z_pres, the p_z its count-prior KL stored,
 *   the posterior means and standard deviations, the workspace's cell-to-row table, the priors of `d`); x that forward's image, recon
 *   what it returned.  Writes nothing into the workspace.
 * Both return SPAIR_ERR_SHAPE before any launch for a NULL mandatory pointer, B < 1, HW outside [1, 1024], A < 1 or A + 5 > 64, C < 1,
 *   I < 1 or Iw < 1, a leading dimension below its column count. */
long long spair_sample_terms_scratch_floats(int B, int HW, int I, int Iw);
int spair_sample_terms_rows(const float* z_pres, int ld_z, const float* p_z, int ld_pz, const float* mu_box, int ld_mu_box,
                            const float* sd_box, int ld_sd_box, const float* mu_attr, int ld_mu_attr, const float* sd_attr, int ld_sd_attr,
                            const float* mu_depth, int ld_mu_depth, const float* sd_depth, int ld_sd_depth, const int* cidx,
                            const float* prior_mean, const float* prior_std, float beta, const float* recon, const float* x, int B, int HW,
                            int A, int C, int I, int Iw, float* terms, float* kl_map, float* bce_map, float* scratch, int accumulate,
                            float scale, void* stream);
int spair_eval_terms(const SpairDims* d, const void* workspace, int flags, const float* x, const float* recon, float beta, float* terms,
                     float* kl_map, float* bce_map, float* scratch, int accumulate, float scale, void* stream);
/* ---- instance masks of the synthetic scenes (csrc/scenes.hip): spair_scenes_generate with one more output, mask int32 [B][I][I]:
 * mask[b][y][x] = the index j of the glyph whose value at the pixel is largest (the lowest j on a tie), -1 where the pixel is 0.  image,
 * bbox and count are bit for bit what spair_scenes_generate writes; mask >= 0 exactly where image > 0, and mask < count[b].  The same
 * refusals, and SPAIR_ERR_SHAPE for a NULL mask, before any launch. */
int spair_scenes_generate_masks(uint64_t seed, long long first, int B, int I, int K, int size_min, int size_max, float* image,
                                float* bbox, long long* count, float* scratch, int* mask, void* stream);
/* ---- segmentation metrics (csrc/segmentation.hip): a predicted label map scored against a true one, per image, on the device.
 * pred [B][HW] in {-1, 0 .. NP-1}, truth [B][HW] in {-1, 0 .. K-1}; -1 is background, and so is every label outside its range.
 *   contingency [B][NP+1][K+1] (written whole): n[i][j] = pixels with pred = i - 1 and truth = j - 1 (index 0: background); a_i its
 *       row sums, b_j its column sums, N = HW, C2(v) = v (v - 1) / 2.
 *   scores [B][5]:
 *     0 ari:    (X - E) / (M - E) with X = sum C2(n_ij), E = sum C2(a_i) sum C2(b_j) / C2(N), M = (sum C2(a_i) + sum C2(b_j)) / 2;
 *               1 where M = E (both partitions trivial, or N = 1);
 *     1 ari_fg: the same on the columns j >= 1 (pixels of truth objects; background pred pixels are one cluster); NaN without such a pixel;
 *     2 msc, 3 sc: with best_j = max over i >= 1 of n_ij / (a_i + b_j - n_ij) for every object j >= 1 with b_j > 0 (0 if no segment
 *               meets it): their mean, and their mean weighted by b_j; NaN if no object has a pixel;
 *     4 fg_iou: |pred >= 0 and truth >= 0| / |pred >= 0 or truth >= 0|, 1 if both are empty.
 *   match [B][K] (may be NULL): the lowest predicted label attaining best_j > 0, else -1; match_iou [B][K] (may be NULL): best_j (0
 *       for an object without pixels).  Candidates are compared by 64-bit cross-multiplication: no division decides a match.
 * Sums are exact integers (the score numerators and denominators 128-bit), converted to double once and stored as fp32.  Integer
 * atomics only: bit-identical from run to run.  A memset and two launches on `stream`; no allocation, no host synchronisation.
 * SPAIR_ERR_SHAPE before any launch for B < 1, HW outside [1, 2^24], NP outside [1, 1024], K outside [1, 32], a NULL pred, truth,
 * contingency or scores. */
int spair_segmentation(const int* pred, const int* truth, int B, long long HW, int NP, int K, int* contingency, float* scores,
                       int* match, float* match_iou, void* stream);
/* ---- detection metrics (csrc/detection.hip): predicted boxes with scores against the true boxes of each image, on the device: ranked,
 * matched greedily one-to-one at every IoU threshold, and the precision / recall curve pooled over all the images fed.
 * Per image b: predictions n = 0 .. N-1 with boxes [B][N][4] = (x0, y0, x1, y1) in pixels (true corners, as parse_boxes gives them --
 *   not the top-left reading of spair_metrics) and scores [B][N]; truths j = 0 .. K-1 with bbox [B][K][4] = (x, y, w, h) in pixels (the
 *   scene generator's format; corners x, y, x + w, y + h, each sum rounded once), of which the first cnt[b] = clamp(count[b], 0, K)
 *   are real; thresholds [T] in fp32.  1 <= N <= 1024, 1 <= K <= 32, 1 <= T <= 16, 1 <= max_det <= N, min_score finite.
 * IoU of boxes a, b, in fp32, one rounding per operation and no contraction:
 *     iw = max(min(ax1, bx1) - max(ax0, bx0), 0), ih likewise;  inter = iw * ih;
 *     ua = (ax1 - ax0) * (ay1 - ay0), ub likewise;  un = (ua + ub) - inter;  iou = un > 0 ? inter / un : 0;
 *   and +0 where that is not above 0 (an empty intersection, a NaN) or where any of the eight coordinates is NaN or infinite.
 * Live: a prediction whose score is no NaN and >= min_score; n_pred[b] = the number of live predictions, before any cap.
 * Ranked list: the live predictions by score descending (-0 = +0), equal scores by lower n first; only the first
 *   kept = min(n_pred, max_det) enter the matching (COCO's maxDets).
 * Matching, for every threshold t on its own: walk the ranked list in order; among the real truths not yet taken at t choose the one
 *   with the largest IoU, on equal IoU the lowest j; if that IoU >= thresholds[t] (an fp32 compare) the prediction is a true positive at t
 *   and takes the truth, otherwise (or with no truth left) a false positive at t.  Bit t of the prediction's tp word is the outcome.
 * spair_det_match (one launch on `stream`) writes, with a fixed stride of max_det slots per image at the caller's row pointers,
 *   score [B][max_det], tp [B][max_det], order [B][max_det] (the prediction's index n) in ranked order, dead slots -inf / 0 / -1;
 *   n_pred [B], n_truth [B] (= cnt); iou [B][N][K] (may be NULL: not touched; else written whole, all K truth slots as given); and ADDS
 *   to counters[SPAIR_DET_COUNTERS] (64-bit, caller-zeroed, integer atomics: exact and order-independent): 0 sum of cnt, 1 sum of kept
 *   (the records), 2 images with n_pred == cnt, 3 sum of |n_pred - cnt|, 4 sum of n_pred - cnt, 5 images, 6 .. 7 unused,
 *   8 + t the true positives at threshold t.
 * Pooled curve: the records (score, tp word) in insertion order -- image by image as fed, ranked order inside an image -- sorted by score
 *   descending, STABLY (the caller's sort; dead slots, -inf, come last).  For threshold t, over the M = counters[1] records:
 *     TP_i = records 0 .. i with bit t set, prec_i = TP_i / (i + 1), NT = counters[0];
 *     AP_t = (1 / NT) sum over the records i with bit t set of max_{k >= i} prec_k (the area under the precision envelope, all points);
 *     NaN if NT = 0, 0 without a record;  recall_t = TP_last / NT (NaN if NT = 0);  precision_t = TP_last / M (NaN if M = 0).
 *   Counts are exact integers; the divisions and the sum are float64, the sum in an order fixed by M alone.
 * spair_det_ap (one launch on `stream`, no atomics: bit-identical from run to run): tp_sorted [M_slots] the tp words in sorted order,
 *   counters the block above (read on the device: counters[1] is clamped to M_slots), out double [3][T] = AP, recall, precision.
 * Count statistics over the images fed, from the integer sums: count_accuracy = counters[2] / counters[5], count_mae = counters[3] /
 *   counters[5], count_bias = counters[4] / counters[5].
 * Both: no allocation, no host synchronisation.  SPAIR_ERR_SHAPE before any launch for B < 1, N, K, T or max_det outside the limits
 *   above, a NaN or infinite min_score, M_slots outside [1, 2^31 - 1], a NULL pointer other than iou. */
#define SPAIR_DET_COUNTERS 24
int spair_det_match(const float* boxes, const float* scores, const float* bbox, const int* count, const float* thresholds, int B, int N,
                    int K, int T, float min_score, int max_det, float* score, int* tp, int* order, int* n_pred, int* n_truth,
                    long long* counters, float* iou, void* stream);
int spair_det_ap(const int* tp_sorted, long long M_slots, int T, const long long* counters, double* out, void* stream);
/* ---- gradient norm and clipping by global L2 norm (csrc/gradnorm.hip; torch.nn.utils.clip_grad_norm_ in front of the Adam of
 * train.py:44, which the reference itself never calls).  The norm is taken over SEGMENTS of the flat gradient buffer -- nseg ascending,
 * non-overlapping, non-empty element ranges [seg_lo[s], seg_hi[s]), gaps allowed and never read -- cut into WORK ITEMS (segment, lo, hi) of at
 * most SPAIR_GRAD_CHUNK consecutive floats inside one segment.  Every element is converted to float64 BEFORE it is squared and every
 * sum is float64, so the norm of a buffer of 1e30s or of 1e-30s is its true norm, not inf or 0.  The order of every sum is fixed by
 * the table and the buffer's address (per lane strided, a cross-lane tree, the four waves in order; a segment's items in item order;
 * the segments in segment order).  No atomics: bit-identical from run to run.
 * spair_grad_norm_items (host only, touches no GPU): returns the number of work items of the segment table, and with items != NULL writes
 *   items[3 k .. 3 k + 2] = {segment, lo, hi}, segments in order, pieces in order.  SPAIR_ERR_SHAPE for n <= 0, nseg outside
 *   [1, SPAIR_GRAD_MAX_SEGMENTS], a NULL seg_lo / seg_hi, an empty, descending or overlapping segment, a segment past n.
 * spair_grad_norm (two launches on `stream`): items_dev: that table on the device; partial: double[n_items] (one per item, written);
 *   seg_sumsq: double[nseg] (the squared norm per segment, written); out: float[2] = {norm, scale}, norm = (float)sqrt(total) and
 *   scale = fminf(1, max_norm / (norm + norm_eps)) in fp32 when max_norm > 0 and the norm is finite, else exactly 1; clip: int[2]
 *   (caller-zeroed, accumulating) = {calls with scale < 1, calls with a non-finite norm}.  max_norm <= 0: measure only.  Nothing is
 *   written to grads.  SPAIR_ERR_SHAPE before any launch for a NULL pointer, n_items < nseg or >= 2^31, nseg outside
 *   [1, SPAIR_GRAD_MAX_SEGMENTS], norm_eps < 0 or NaN, a NaN max_norm.  The table is trusted (it is spair_grad_norm_items' output).
 * spair_adam_clipped: spair_adam_guarded on gradients scaled by norm_out[1] (spair_grad_norm's out, read on the device): gi = g[i] * scale
 *   in place of g[i], in the per-element guard as well; grads is NOT written.  A non-finite norm_out[0] leaves the whole step out --
 *   parameters and moments untouched, counters untouched (clip[1] counted it).  With scale == 1 the result is bit-identical to
 *   spair_adam_guarded's.  SPAIR_ERR_SHAPE for n <= 0, step < 1, a NULL params / grads / exp_avg / exp_avg_sq / counters / norm_out. */
#define SPAIR_GRAD_CHUNK 4096
#define SPAIR_GRAD_MAX_SEGMENTS 4096
int spair_grad_chunk(void);
long long spair_grad_norm_items(const int64_t* seg_lo, const int64_t* seg_hi, int nseg, int64_t n, int64_t* items);
int spair_grad_norm(const float* grads, const int64_t* items_dev, long long n_items, int nseg, double* partial, double* seg_sumsq,
                    float* out, float max_norm, float norm_eps, int* clip, void* stream);
int spair_adam_clipped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                       float eps, int step, const int* skip, int* counters, const float* norm_out, void* stream);
#ifdef __cplusplus
}
#endif
