/* C ABI of libmonosdf_hip.so -- the gfx950 (MI355X) implementation of MonoSDF's SDF
 * volume-rendering hot path.  Plain C: raw DEVICE pointers, sizes, an explicit
 * hipStream_t passed as void*; every function returns 0 on success (see MSDF_* codes).
 * Callers own every buffer; nothing here allocates, frees or synchronises.
 *
 * What each entry point replaces in the reference (paths relative to /root/reference/code):
 *
 *   msdf_hash_encode_forward / _backward / _second_backward
 *       the pybind11 module `_hash_encoder` (hashencoder/src/bindings.cpp:5-8,
 *       hashencoder/src/hashencoder.h:13-15): same argument order and meaning, tensors
 *       replaced by device pointers, plus the stream the reference never passed.
 *   msdf_pack_weights, msdf_sdf_forward, msdf_sdf_fwd_grad, msdf_sdf_backward
 *       ImplicitNetwork / ImplicitNetworkGrid .forward / .get_sdf_vals / .get_outputs /
 *       .gradient_sdf and their autograd double backward (model/network.py:79-137, 247-309).
 *   msdf_color_forward, msdf_color_backward
 *       RenderingNetwork.forward and its backward (model/network.py:389-470).
 *   msdf_wgrad, msdf_reduce
 *       the dW / db `mm` + `sum` nodes autograd emits for those networks
 *       (implied by loss.backward(), training/monosdf_train.py:431).
 *   msdf_composite_forward, msdf_composite_backward
 *       LaplaceDensity (model/density.py:21-30), MonoSDFNetwork.volume_rendering and the
 *       composites (model/network.py:552-562, 603-605, 626-640) and their backward.
 *   msdf_sampler_* (see below)
 *       ErrorBoundSampler.get_z_vals / UniformSampler.get_z_vals (model/ray_sampler.py:48-83, 110-272).
 *   msdf_weightnorm_forward, msdf_weightnorm_backward
 *       the nn.utils.weight_norm hooks of every Linear (model/network.py:72-73, 239-240, 381-382).
 *   msdf_camera_rays
 *       rend_util.get_camera_params + lift, called twice per chunk (utils/rend_util.py:63-91, 105-118;
 *       model/network.py:505-516).
 *   msdf_pixel_rays
 *       the dataset's per-pixel ray tables and the pixel branch of its __getitem__ (datasets/scene_dataset.py:269-307,
 *       374-401).
 *   msdf_monosdf_loss
 *       MonoSDFLoss.forward and its backward (model/loss.py:180-311 with 29-87, 156-171).
 *   msdf_probe_loss
 *       no reference counterpart: the fixed scalar bench.py differentiates.
 *   msdf_mc_workspace_bytes, msdf_mc_count, msdf_mc_emit
 *       skimage.measure.marching_cubes as get_surface_sliding calls it (utils/plots.py:199-205).
 *   msdf_nn_split_count, msdf_nn_workspace_bytes, msdf_nn_search
 *       the all-nearest-neighbour queries of the mesh evaluation scripts: sklearn KDTree(...).query
 *       (scannet_eval/evaluate.py:16-26) and scipy cKDTree(...).query (replica_eval/eval_recon.py:25-43, 96-106).
 *   msdf_voxel_keys, msdf_voxel_mean
 *       open3d PointCloud.voxel_down_sample as evaluate() calls it (scannet_eval/evaluate.py:36-38); the sort between
 *       the two calls is the caller's.
 *
 * Entry points that take an msdf_plan_t run on the matrix core named by plan->precision (monosdf_plan.h).
 */
#ifndef MONOSDF_HIP_H
#define MONOSDF_HIP_H

#include <stdint.h>
#include "monosdf_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSDF_OK 0
#define MSDF_ERR_ARG 1
#define MSDF_ERR_LAUNCH 2
#define MSDF_ERR_UNSUPPORTED 3

#define MSDF_ABI_VERSION 8
int msdf_abi_version(void);

/* ---- hash grid (reference: hashencoder/src/hashencoder.h:13-15) ----
 * calc_grad_inputs: 0 / 1 as in the reference (dy_dx laid out [B, L, 3 C]); 2 = the same with dy_dx level-major
 * [L, B, 3 C], which every kernel here reads and writes as contiguous rows -- a caller that owns dy_dx end to end
 * passes 2 to all three calls.
 *
 * Return codes of the seven entry points that produce a table (embedding) gradient -- msdf_hash_encode_backward,
 * _second_backward, _backward_ws, _second_backward_ws, _backward_fused, _backward_fused_out, msdf_hash_node_scatter.
 * The tests are made in this order, the first that fails decides, and a refused call launches nothing: the table
 * gradient is left untouched.
 *
 *   1  D != 3 (entries that take D)                                          MSDF_ERR_UNSUPPORTED
 *   2  C not 1, 2, 4 or 8; C == 1 in anything second-order (every entry
 *      but _backward and _backward_ws: the reference has none either)        MSDF_ERR_UNSUPPORTED
 *   3  _fused, _fused_out: grad_embeddings, grad_first, grad_second or
 *      grad_grad_inputs NULL; node_scatter: grad_embeddings NULL             MSDF_ERR_ARG
 *   4  B == 0: nothing is read, the other pointers may be NULL               MSDF_OK
 *      ("=" forms, _fused_out and node_scatter: the table gradient is set to zero; "+=" forms: untouched)
 *   5  a NULL operand of a requested output (below); pitch != 0 and
 *      pitch < L*C (node_scatter)                                            MSDF_ERR_ARG
 *   6  a table of n_entries*C >= 2^31 floats or B*L*8 >= 2^31 corner
 *      records (the binned entries: all but _backward, _second_backward)     MSDF_ERR_UNSUPPORTED
 *   7  workspace NULL, not 16-byte aligned, or shorter than
 *      msdf_hash_scatter_workspace_bytes(B, C, L, n_entries)                 MSDF_ERR_ARG
 *
 * Outputs and operands of the four reference-order entries: a NULL grad_embeddings / grad2_embeddings / grad_grad
 * skips that output (calc_grad_inputs == 0 skips grad_inputs), and with it the workspace is not looked at.  The table
 * gradient needs grad, inputs, offsets (and grad_grad_inputs, second order); grad_inputs needs grad and dy_dx;
 * grad_grad needs grad_grad_inputs and dy_dx.  node_scatter needs its three operands, inputs and offsets.
 * `embeddings` is never read.  MSDF_ERR_LAUNCH: the runtime refused a launch.
 *
 * Return codes of the entry points that read the table or its Jacobian -- msdf_hash_encode_forward, the grad_inputs
 * part of msdf_hash_encode_backward and the grad_grad part of msdf_hash_encode_second_backward (grad_embeddings /
 * grad2_embeddings NULL), msdf_hash_node_forward, msdf_hash_node_input_gradient, msdf_hash_node_second_grad,
 * msdf_hash_transpose.  Again in this order, the first that fails decides, and a refused call launches nothing: the
 * outputs are left untouched.
 *
 *   1  D != 3 (entries that take D); _backward and _second_backward:
 *      their row 2 above as well, before B is looked at                      MSDF_ERR_UNSUPPORTED
 *   2  B == 0: nothing is read, every pointer may be NULL -- also with a
 *      C, pitch, n_split or L*C that rows 3 to 5 would refuse                MSDF_OK
 *   3  a NULL required operand (below); pitch != 0 and pitch < L*C (node
 *      forms; transpose: pitch < L*C, pitch 0 included); n_split > B
 *      (node_second_grad); transpose: L*C == 0, or only one of src2 / dst2   MSDF_ERR_ARG
 *   4  node_input_gradient: 3*B >= 2^32;
 *      transpose: an LDS tile 64*(L*C + 1)*4 bytes > 64 KiB (L*C > 255)      MSDF_ERR_UNSUPPORTED
 *   5  C not 1, 2, 4 or 8 (all but transpose, which takes any C)             MSDF_ERR_UNSUPPORTED
 *
 * Required operands.  _forward: inputs, embeddings, offsets, outputs, and dy_dx unless calc_grad_inputs == 0 (then
 * dy_dx is neither read nor written).  _backward with calc_grad_inputs != 0: grad, dy_dx, grad_inputs;
 * _second_backward with grad_grad given: grad_grad_inputs, dy_dx.  node_forward: x, embeddings, offsets, feat
 * (x01_out and dy_dx may be NULL: not written).  node_input_gradient: g, dy_dx, inout.  node_second_grad: gg_out,
 * dy_dx, grad_grad (g_a and g_b may each be NULL: that part of gg_out is zero).  transpose: src, dst. */
int msdf_hash_encode_forward(const float* inputs, const float* embeddings, const int* offsets, float* outputs,
                             uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                             int calc_grad_inputs, float* dy_dx, void* stream);
int msdf_hash_encode_backward(const float* grad, const float* inputs, const float* embeddings, const int* offsets,
                              float* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                              uint32_t H, int calc_grad_inputs, const float* dy_dx, float* grad_inputs,
                              void* stream);
int msdf_hash_encode_second_backward(const float* grad, const float* inputs, const float* embeddings,
                                     const int* offsets, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                     uint32_t H, int calc_grad_inputs, const float* dy_dx,
                                     const float* grad_grad_inputs, float* grad_grad, float* grad2_embeddings,
                                     void* stream);

/* The same two gradients with the embedding scatter summed per table slice in LDS instead of one memory-side float
 * atomic per corner (csrc/hash_scatter.h "Binned scatter"): the argument lists above, followed by the number of rows of
 * the embedding table and a caller-owned DEVICE workspace of at least msdf_hash_scatter_workspace_bytes() bytes
 * (16-byte aligned; contents are scratch, nothing persists between calls).  Results equal the plain entry points up
 * to the order of the fp32 sums. */
int64_t msdf_hash_scatter_workspace_bytes(uint32_t B, uint32_t C, uint32_t L, uint64_t n_entries);
int msdf_hash_encode_backward_ws(const float* grad, const float* inputs, const float* embeddings, const int* offsets,
                                 float* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                 uint32_t H, int calc_grad_inputs, const float* dy_dx, float* grad_inputs,
                                 uint64_t n_entries, void* workspace, uint64_t workspace_bytes, void* stream);
int msdf_hash_encode_second_backward_ws(const float* grad, const float* inputs, const float* embeddings,
                                        const int* offsets, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                        uint32_t H, int calc_grad_inputs, const float* dy_dx,
                                        const float* grad_grad_inputs, float* grad_grad, float* grad2_embeddings,
                                        uint64_t n_entries, void* workspace, uint64_t workspace_bytes, void* stream);
/* Both embedding gradients of a training step in one scatter (they visit the same corners): grad_embeddings +=
 * what msdf_hash_encode_backward adds for `grad_first` plus what msdf_hash_encode_second_backward adds for
 * (`grad_second`, grad_grad_inputs).  grad_first / grad_second: [L,B,C]. */
int msdf_hash_encode_backward_fused(const float* grad_first, const float* grad_second, const float* inputs,
                                    const int* offsets, float* grad_embeddings, uint32_t B, uint32_t D, uint32_t C,
                                    uint32_t L, float S, uint32_t H, const float* grad_grad_inputs,
                                    uint64_t n_entries, void* workspace, uint64_t workspace_bytes, void* stream);
/* The same with "=" instead of "+=": grad_embeddings is an output and need not be initialised by the caller (the
 * reference's callers zero-fill it first, hashgrid.py:75-76,93-94: here neither that fill nor a read of the table
 * is needed). */
int msdf_hash_encode_backward_fused_out(const float* grad_first, const float* grad_second, const float* inputs,
                                        const int* offsets, float* grad_embeddings, uint32_t B, uint32_t D, uint32_t C,
                                        uint32_t L, float S, uint32_t H, const float* grad_grad_inputs,
                                        uint64_t n_entries, void* workspace, uint64_t workspace_bytes, void* stream);

/* "Node" forms for the fused grid node (no counterpart in the reference: it runs these steps as tensor expressions
 * around its three kernels).  Points in world coordinates: x01 = (x / divide_factor + 1) / 2 is formed inside, rounded
 * as the tensor expression rounds it, and returned in x01_out (may be NULL).  Features and the gradients with respect
 * to them: pitch == 0 level-major [L, B, C] (the hash kernels' own, coalesced layout); pitch > 0 point-major rows of
 * `pitch` floats ([B, pitch], level l channel c at column l*C + c, columns >= L*C written as zeros) -- what the fused
 * SDF kernels read / write.  dy_dx is level-major [L, B, 3C] (NULL: none).
 * msdf_hash_transpose: [L, B, C] <-> [B, pitch] through LDS tiles (both sides coalesced), one or two tensors per launch.
 * msdf_hash_node_input_gradient: inout[b,:] += scale * sum_{l,c} g(b,l,c) * dy_dx[l,b,:,c].
 * msdf_hash_node_second_grad: gg_out[b,:] = scale * (b < n_split ? g_a[b,:] : g_b[b - n_split,:]) (NULL part = 0),
 * grad_grad[b, l*C+c] = sum_d gg_out[b,d] * dy_dx[l,b,d,c].
 * msdf_hash_node_scatter: msdf_hash_encode_backward_fused_out with point-major grad_first / grad_second. */
int msdf_hash_node_forward(const float* x, double divide_factor, float* x01_out, const float* embeddings,
                           const int* offsets, float* feat, uint32_t pitch, uint32_t B, uint32_t C, uint32_t L,
                           float S, uint32_t H, float* dy_dx, void* stream);
int msdf_hash_node_input_gradient(const float* g, uint32_t pitch, const float* dy_dx, uint32_t B, uint32_t C,
                                  uint32_t L, float scale, float* inout, void* stream);
int msdf_hash_node_second_grad(const float* g_a, const float* g_b, uint32_t n_split, float scale, float* gg_out,
                               const float* dy_dx, float* grad_grad, uint32_t pitch, uint32_t B, uint32_t C,
                               uint32_t L, void* stream);
int msdf_hash_transpose(const float* src, float* dst, const float* src2, float* dst2, uint32_t L, uint32_t B,
                        uint32_t C, uint32_t pitch, int to_point_major, void* stream);
int msdf_hash_node_scatter(const float* grad_first, const float* grad_second, uint32_t pitch, const float* inputs,
                           const int* offsets, float* grad_embeddings, uint32_t B, uint32_t C, uint32_t L, float S,
                           uint32_t H, const float* grad_grad_inputs, uint64_t n_entries, void* workspace,
                           uint64_t workspace_bytes, void* stream);

/* ---- fused MLPs ----
 * Every entry point that takes a plan runs on the matrix core named by plan->precision (monosdf_plan.h):
 * MSDF_PRECISION_F32 = fp32 MFMA; MSDF_PRECISION_BF16X3 = each product as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi
 * on the bf16 matrix cores with fp32 accumulation (~1e-5 relative error, measured in tests/); MSDF_PRECISION_BF16X6 =
 * three bf16 planes per operand and the six cross terms down to 2^-16 of the product (fp32-grade: its parity tests
 * are held to the fp32 core's tolerances; msdf_wgrad runs the fp32 kernel for it).  The cores use
 * different weight packs: `wpack` is opaque, sized by the host (monosdf_amd/plan.py) and produced by
 * msdf_pack_weights for the same plan. */
int msdf_pack_weights(const msdf_plan_t* plan, const msdf_packrule_t* rules_dev, const int* maps_dev,
                      const float* flat_w, const float* flat_b, void* wpack, float* bpack, void* stream);

/* weight normalisation of every layer of a network in one launch (reference: nn.utils.weight_norm hooks,
 * model/network.py:72-73, 239-240, 381-382).  row_layer_dev[r] = layer index of global row r. */
typedef struct {
  const float* v;      /* [rows, cols] weight_v (or the plain weight when has_g == 0) */
  const float* g;      /* [rows] weight_g */
  const float* b;      /* [rows] bias */
  int32_t rows, cols;
  int32_t w_off;       /* float offset of this layer in the flat weight buffer */
  int32_t b_off;       /* float offset of this layer in the flat bias buffer */
  int32_t row_off;     /* first global row of this layer */
  int32_t has_g;
} msdf_wn_layer_t;
int msdf_weightnorm_forward(const msdf_wn_layer_t* layers_dev, const int* row_layer_dev, int total_rows,
                            float* flat_w, float* flat_b, float* norms, void* stream);
int msdf_weightnorm_backward(const msdf_wn_layer_t* layers_dev, const int* row_layer_dev, int total_rows,
                             const float* g_flat_w, const float* norms, float* dv_flat, float* dg_rows, void* stream);

int msdf_sdf_forward(const msdf_plan_t* plan, const void* wpack, const float* bpack, const float* x,
                     const float* aux, int P, float clamp_radius, float sphere_scale, float* sdf, void* stream);
/* the same, skipped on the device when *run_flag == 0 (run_flag may be NULL): the SDF evaluation of a sampler round
 * that the previous round did not ask for (msdf_sampler_args_t.flags) costs a kernel start, not a network pass */
int msdf_sdf_forward_if(const msdf_plan_t* plan, const void* wpack, const float* bpack, const float* x,
                        const float* aux, int P, float clamp_radius, float sphere_scale, float* sdf,
                        const uint32_t* run_flag, void* stream);
/* the same with the extra input features given as the hash encoder's level-major tensor [aux_LC / aux_C][P][aux_C]
 * (msdf_fg_args_t.aux_C); aux_C == 0 is msdf_sdf_forward_if */
int msdf_sdf_forward_lm(const msdf_plan_t* plan, const void* wpack, const float* bpack, const float* x,
                        const float* aux, int aux_C, int aux_LC, int P, float clamp_radius, float sphere_scale,
                        float* sdf, const uint32_t* run_flag, void* stream);
/* msdf_sdf_forward_lm (bit-identical sdf) for P = rays * n_cols points, point ray * n_cols + c, that also stores the
 * post-activation of every hidden layer of the points whose column c has col_slot[c] >= 0 (col_slot: n_cols entries on
 * the device) to row ray * n_slots + col_slot[c] of H, laid out as the H of an msdf_sdf_fwd_grad launch with P_pad
 * rows: the staging buffer (h_stage, stage_pad) of the launch that may then skip the hidden layers of those points
 * (msdf_fg_args_t.n_reuse).  Sets *h_saved = 1.
 * fp32 core only (MSDF_ERR_UNSUPPORTED otherwise). */
int msdf_sdf_forward_save(const msdf_plan_t* plan, const void* wpack, const float* bpack, const float* x,
                          const float* aux, int aux_C, int aux_LC, int P, float clamp_radius, float sphere_scale,
                          float* sdf, const uint32_t* run_flag, float* H, int P_pad, const int32_t* col_slot,
                          int n_cols, int n_slots, uint32_t* h_saved, void* stream);

typedef struct {
  const void* wpack;
  const float* bpack;
  const float* x;          /* [P,3] */
  const float* aux;        /* [P, 16*aux_tiles] or NULL */
  int32_t P, P_pad;        /* P_pad = P rounded up to 64 (workspace rows) */
  int32_t n_clamp;         /* points [0,n_clamp) get the bounding-sphere clamp */
  int32_t n_feat;          /* points [0,n_feat) need the feature vector (multiple of 16 or == P) */
  float clamp_radius, sphere_scale;
  float* sdf;              /* [P] */
  float* feat;             /* [n_feat, 16*feat_tiles] */
  float* nrm;              /* [P,3] */
  float* r_aux;            /* [P, 16*aux_tiles] or NULL */
  unsigned char* clamped;  /* [P] */
  float* H;                /* [hsum * P_pad] */
  float* PM;               /* [hsum * P_pad] */
  float* IN0;              /* [P_pad, 16*(e_tiles+aux_tiles)] */
  int32_t save;
  int32_t aux_C;           /* layout of aux / r_aux: 0 = rows [P, 16*aux_tiles]; C = 1, 2, 4, 8: the hash encoder's own
                              level-major tensors [aux_LC / C][P][C] (column l C + c of a point = level l, channel c) */
  int32_t aux_LC;          /* valid columns (levels x channels) of the level-major form */
  float aux_dx_scale;      /* with dy_dx: the chain-rule factor of x -> x01 (0.5 / divide_factor) */
  const float* dy_dx;      /* NULL, or (aux_C == 2 only) the hash encoder's Jacobian [L][P][3][2] as
                              msdf_hash_node_forward writes it: nrm then also holds the grid part of d sdf / d x,
                              nrm += aux_dx_scale * sum_{l,c} r_aux[l,c] dy_dx[l,.,c] (what msdf_hash_node_input_gradient
                              adds as a launch of its own; reference kernel_input_backward, hashencoder.cu:346-372) */
  /* Evaluation order != row order (fp32 core only; the bf16 cores ignore these fields).  The point evaluated at row r
   * of the launch grid is row row_map[r] of every tensor AND of the workspace (a permutation of [0, P) that maps
   * [n_feat, P) and [n_clamp, P) to themselves): which workgroup evaluates a point changes, nothing that is read or
   * written does.  NULL = identity. */
  const int32_t* row_map;
  /* Reuse of hidden activations that msdf_sdf_forward_save staged in h_stage (rows in evaluation order, stage_pad rows
   * per layer block): a workgroup whose 64 evaluation rows lie below n_reuse (a multiple of 64, <= stage_pad) skips
   * the hidden layers' forward products -- it takes the activations from the staged rows and stores them to the
   * points' own rows of H on the way -- if and only if smp_flags[1] == 0 (the sampler stopped after its first round)
   * and *h_saved != 0 (the save ran).  Decided on the device, per workgroup; n_reuse == 0 or a NULL pointer:
   * everything is computed. */
  const uint32_t* smp_flags;
  const uint32_t* h_saved;
  int32_t n_reuse;
  int32_t stage_pad;
  const float* h_stage;
  /* Dispatch rotation (fp32 core only; MSDF_ERR_UNSUPPORTED if non-zero on a bf16 core): block b of the launch
   * evaluates workgroup (b + wg_first) mod n_wg, n_wg = P_pad / 64, so that workgroup wg_first is the first the
   * hardware starts and wg_first - 1 the last.  With n_reuse > 0, wg_first = n_reuse / 64 starts the workgroups that
   * compute everything before the shorter reusing ones.  0 <= wg_first < n_wg.  Changes the order in which workgroups
   * start and nothing else: every workgroup evaluates, reads and writes the rows it does with 0. */
  int32_t wg_first;
} msdf_fg_args_t;
int msdf_sdf_fwd_grad(const msdf_plan_t* plan, const msdf_fg_args_t* args, void* stream);

typedef struct {
  const void* wpack;
  const float* bpack;
  const float* x;
  int32_t P, P_pad;
  int32_t n_feat;
  int32_t n_split;         /* points [0, n_split) take g_sdf / g_nrm, points [n_split, P) take g_sdf_b / g_nrm_b:
                              the two groups (ray samples | eikonal points) get their gradients from different
                              consumers, and this spares the caller the zero-fill + copy + add of joining them */
  const float* g_sdf;      /* [n_split] or NULL */
  const float* g_feat;     /* [n_feat, 16*feat_tiles] or NULL */
  const float* g_nrm;      /* [n_split,3] or NULL */
  const float* g_raux;     /* [P, 16*aux_tiles] or NULL */
  const unsigned char* clamped;
  const float* H;
  const float* PM;
  float* QB;               /* [qsum * P_pad] */
  float* T;                /* unused (may be NULL): the second-order term 100 (1 - s) p p-bar is formed again in the
                              sweep down from PM and the stored q-bar rows instead of being written and re-read */
  float* AB;               /* [absum * P_pad] */
  float* GSDF;             /* [P_pad] */
  float* QLAST;            /* [P_pad, 16*kt_last] */
  float* g_aux;            /* [P, 16*aux_tiles] or NULL */
  const float* g_sdf_b;    /* [P - n_split] or NULL */
  const float* g_nrm_b;    /* [P - n_split, 3] or NULL */
  int32_t aux_C, aux_LC;   /* layout of g_raux / g_aux, as in msdf_fg_args_t */
  const float* dy_dx;      /* NULL, or (aux_C == 2 only) the encoder's Jacobian [L][P][3][2]: the gradient arriving at
                              d sdf / d features from the grid part of d sdf / d x is then formed in the kernel from
                              g_nrm, g_raux[l,c] = sum_d (aux_dx_scale g_nrm[d]) dy_dx[l,d,c] (g_raux itself is ignored) --
                              what msdf_hash_node_second_grad computes as a launch of its own (reference
                              kernel_grid_second_backward_grad, hashencoder.cu:375-428), bit-identical to it */
  float* gg_out;           /* with dy_dx: [P,3] <- aux_dx_scale * g_nrm (the scatter's grad_grad_inputs), or NULL */
  float aux_dx_scale;
  int32_t pad_;
  const int32_t* row_map;  /* as in msdf_fg_args_t (the same map as the forward + gradient launch, or NULL): grid row r
                              works on row row_map[r] of every tensor and of the workspace */
} msdf_bw_args_t;
int msdf_sdf_backward(const msdf_plan_t* plan, const msdf_bw_args_t* args, void* stream);

typedef struct {
  const void* wpack;
  const float* bpack;
  const float* x;          /* [P,3] */
  const float* dirs;       /* [P/spr,3] */
  const float* nrm;        /* [P,3] */
  const float* feat;       /* [P, 16*feat_tiles] */
  const float* code;       /* [P/spr, 16*aux_tiles] or NULL */
  int32_t P, P_pad;
  int32_t spr;             /* samples per ray */
  int32_t save;
  float* rgb;              /* [P,3] */
  float* H;                /* [n_hidden][P_pad][16*hid_tiles] */
  float* MISC;             /* [P_pad, 16*misc_tiles] */
} msdf_color_fwd_args_t;
int msdf_color_forward(const msdf_plan_t* plan, const msdf_color_fwd_args_t* args, void* stream);

typedef struct {
  const void* wpack;
  const float* bpack;
  const float* rgb;
  const float* g_rgb;
  int32_t P, P_pad;
  const float* H;
  float* AB;               /* [absum * P_pad] */
  float* g_feat;           /* [P, 16*feat_tiles] */
  float* g_misc;           /* [P, 16*misc_tiles] */
  float* g_nrm;            /* [P,3] or NULL: the normal columns of g_misc again, dense (mode idr) */
} msdf_color_bwd_args_t;
int msdf_color_backward(const msdf_plan_t* plan, const msdf_color_bwd_args_t* args, void* stream);

/* wg_map_dev: int32 pairs (item, split) for each of the n_wgs workgroups (balanced by the host) */
int msdf_wgrad(const msdf_wgrad_item_t* items_dev, const int32_t* wg_map_dev, int n_wgs, float* partials,
               int P_pad, int precision /* MSDF_PRECISION_* */, const float* base0, const float* base1 /* the items'
               operand buffers; base1 may be NULL when no item names it */, void* stream);
int msdf_reduce(const msdf_reduce_rule_t* rules_dev, int n_rules, const int* maps_dev, const float* partials,
                float* dst, void* stream);

/* ---- compositor ---- */
typedef struct {
  const float* z;            /* [N,S] */
  const float* sdf;          /* [N,S] */
  const float* rgb;          /* [N,S,3] */
  const float* nrm;          /* [N,S,3] */
  const float* beta;         /* [1] = |beta| + beta_min */
  const float* depth_scale;  /* [N] with a pitch of depth_scale_stride floats (the z column of a [N,3] direction table) */
  int32_t N, S;
  int32_t white_bkgd;
  float bg0, bg1, bg2;
  float* weights;            /* [N,S] */
  float* rgb_values;         /* [N,3] */
  float* depth_values;       /* [N] */
  float* normal_map;         /* [N,3]: R^T sum_i w_i n_i/(|n_i|+1e-6) (camera frame) when pose != NULL, else world frame */
  float* wsum;               /* [N] */
  const float* pose;         /* [N or 1, 4, 4] camera-to-world matrices or NULL (reference network.py:608-616) */
  int32_t pose_stride;       /* 16 per-ray poses, 0 one pose for all rays */
  int32_t depth_scale_stride; /* floats between the depth scales of consecutive rays (0 is read as 1) */
  float* depth_vals;         /* [N,S] = z * depth_scale (reference network.py:572), or NULL */
} msdf_composite_args_t;
int msdf_composite_forward(const msdf_composite_args_t* args, void* stream);

typedef struct {
  const float* z;
  const float* sdf;
  const float* rgb;
  const float* nrm;
  const float* beta;
  const float* depth_scale;
  const float* weights;
  const float* wsum;
  const float* depth_values;
  const float* g_rgb_values;  /* [N,3] or NULL */
  const float* g_depth;       /* [N] or NULL */
  const float* g_normal;      /* [N,3] or NULL */
  const float* g_weights;     /* [N,S] or NULL */
  int32_t N, S;
  int32_t white_bkgd;
  float bg0, bg1, bg2;
  float* g_sdf;               /* [N,S] */
  float* g_rgb;               /* [N,S,3] */
  float* g_nrm;               /* [N,S,3] */
  float* g_beta_part;         /* [N] */
  const float* pose;          /* as in the forward */
  int32_t pose_stride;
  int32_t depth_scale_stride; /* as in the forward */
} msdf_composite_bwd_args_t;
int msdf_composite_backward(const msdf_composite_bwd_args_t* args, void* stream);

/* LaplaceDensity.get_beta (reference model/density.py:28-30) and its adjoint, one launch each:
 * out[0] = |beta_raw[0]| + beta_min;   g_raw[0] = sign(beta_raw[0]) * sum_i g_part[i]  (fixed summation order). */
int msdf_beta_eff(const float* beta_raw, float beta_min, float* out, void* stream);
int msdf_beta_grad(const float* beta_raw, const float* g_part, int n, float* g_raw, void* stream);

/* ---- fused benchmark loss: the value and all gradients in one launch of one workgroup ---- */
typedef struct {
  const float* rgb;      /* [N,3] rgb_values */
  const float* nrm;      /* [N,3] normal_map */
  const float* depth;    /* [N] depth_values */
  const float* g1;       /* [M,3] grad_theta */
  const float* g2;       /* [M,3] grad_theta_nei */
  int32_t N, M;
  float w_normal, w_depth, w_eik, w_smooth;
  float* g_rgb; float* g_nrm; float* g_depth; float* g_g1; float* g_g2;   /* d loss / d input */
  float* partial;        /* [1] the loss value */
} msdf_probe_loss_args_t;
int msdf_probe_loss(const msdf_probe_loss_args_t* args, void* stream);

/* ---- MonoSDFLoss (reference: model/loss.py:180-311 with loss.py:29-87,156-171), pixel-batch mode,
 * L1 colour loss.  One launch returns the seven scalars of the reference's output dict and the gradients of
 * `loss` with respect to every model output.  The decay factor (loss.py:291-296) is folded into w_depth /
 * w_nl1 / w_ncos by the caller. */
typedef struct {
  const float* rgb;          /* [N,3] rgb_values */
  const float* depth;        /* [N]   depth_values */
  const float* normal;       /* [N,3] normal_map */
  const float* sdf;          /* [N,S] sdf of the ray samples (foreground mask: sign change along the ray) */
  const float* grad_theta;   /* [E,3] or NULL (no eikonal / smoothness terms) */
  const float* grad_nei;     /* [E,3] or NULL */
  const float* rgb_gt;       /* [N,3] */
  const float* depth_gt;     /* [N]   monocular depth cue */
  const float* normal_gt;    /* [N,3] monocular normal cue */
  const float* mask_gt;      /* [N]   > 0.5 = valid pixel */
  int32_t N, S, E;
  int32_t gamma;             /* if_gamma_loss */
  int32_t scale_invariant;   /* if_scale_invariant_depth */
  float w_eik, w_smooth, w_depth, w_nl1, w_ncos;
  float* mask;               /* [N] scratch / output: the combined mask as 0 / 1 */
  float* out;                /* [8]: loss, rgb_loss, eikonal_loss, smooth_loss, depth_loss, normal_l1, normal_cos, sum(mask) */
  float* g_rgb; float* g_depth; float* g_normal; float* g_theta; float* g_nei;   /* d loss / d input */
} msdf_monosdf_loss_args_t;
int msdf_monosdf_loss(const msdf_monosdf_loss_args_t* args, void* stream);

/* ---- error-bounded sampler (reference: model/ray_sampler.py:48-83, 110-272) ---- */
typedef struct {
  const float* ray_o;        /* [N,3] */
  const float* ray_d;        /* [N,3] */
  int32_t N;
  int32_t M;                 /* current number of sorted samples per ray */
  int32_t m_max;             /* row pitch of z / sdf (>= n_eval * max_rounds) */
  int32_t n_eval, n_final, n_extra;
  int32_t round_idx, max_rounds;
  int32_t training;          /* 1: final u from u_final, 0: linspace */
  int32_t beta_iters;
  float near, far, bound;    /* sampler near / far clip, cube half-size (scene_bounding_sphere) */
  float eps, add_tiny;
  float lemma;               /* 1 / (4 log(1 + eps)) */
  const float* beta0;        /* [1] device: |beta| + beta_min */
  float* z;                  /* [N, m_max] sorted sample distances */
  float* sdf;                /* [N, m_max] sdf at those samples */
  float* new_z;              /* [N, n_eval] samples added by the last round */
  const float* new_sdf;      /* [N, n_eval] their sdf (from msdf_sdf_forward) */
  int32_t* new_pos;          /* [N, n_eval] their positions in z */
  float* pts;                /* [N * n_eval, 3] their 3-D points */
  float* beta;               /* [N] */
  uint32_t* flags;           /* [2 * max_rounds], zeroed by msdf_sampler_init: flags[2r] = bits of the
                                batch's max beta after round r, flags[2r+1] = 1 when round r asks for another one.
                                Rounds r > 0 return at once unless flags[2(r-1)+1] is set, so enqueueing more rounds
                                than needed is harmless (reference: ray_sampler.py:125,179). */
  const float* jitter;       /* [N, n_eval] or NULL (eval) */
  const float* u_final;      /* [N, n_final] or NULL */
  float* final_z;            /* [N, n_final] */
  const int64_t* extra_idx;  /* [max_rounds, n_extra]: row k-1 = the columns of the dense set to add to the final set
                                when k rounds ran (the kernel reads k from `flags`; reference: ray_sampler.py:242-247) */
  const int64_t* eik_idx;    /* [N] or NULL */
  float* z_out;              /* [N, n_final + n_extra + 2] */
  float* z_eik;              /* [N] or NULL */
  float* pts_out;            /* [N * S (+ 4 N), 3] or NULL: ray samples, then (training) the eikonal points */
  const float* eik_uniform;  /* [N,3] uniform points in the bounding cube, or NULL (no eikonal block) */
  const float* nei_rand;     /* [2N,3] U[0,1) jitter of the neighbour points (reference network.py:583-594) */
  float* far_out;            /* [N] or NULL: msdf_sampler_init also returns the far bound of the uniform samples */
  int32_t* rounds_out;       /* [1] or NULL: msdf_sampler_finish writes the number of rounds that ran */
  float* dbg_dstar;          /* [N, m_max] or NULL: msdf_sampler_beta writes d* of the M-1 intervals (tests) */
  float* dbg_err0;           /* [N] or NULL: msdf_sampler_beta writes the error bound at beta0 (tests) */
  float* dbg_cdf;            /* [N, m_max] or NULL: msdf_sampler_resample writes the cdf it inverts (tests) */
  const float* eik_u;        /* [N] U[0,1) or NULL: when eik_idx is NULL the eikonal sample of a ray is column
                                floor(u * S) of its final set (reference: torch.randint, ray_sampler.py:254) */
  int32_t eik_unit;          /* 1: eik_uniform holds U[0,1) values, mapped to (2u - 1) * bound here (reference:
                                uniform_(-R, R), network.py:587); 0: it holds the points themselves */
  int32_t pad_;
  int32_t* row_map;          /* [N * S (+ 4 N)] or NULL: msdf_sampler_finish writes the evaluation order of the SDF
                                kernels (msdf_fg_args_t.row_map): evaluation rows [0, n_extra N) are the dense-set
                                columns, row ray * n_extra + e for extra_idx entry e, rows [n_extra N, S N) the other
                                samples of each ray in sorted order, the eikonal rows map to themselves;
                                row_map[r] = the row of pts_out / z_out that evaluation row r is */
  uint32_t* h_saved;         /* [1] or NULL: zeroed by msdf_sampler_init (msdf_sdf_forward_save sets it) */
} msdf_sampler_args_t;
int msdf_sampler_init(const msdf_sampler_args_t* args, void* stream);
int msdf_sampler_beta(const msdf_sampler_args_t* args, void* stream);
int msdf_sampler_resample(const msdf_sampler_args_t* args, void* stream);
int msdf_sampler_finish(const msdf_sampler_args_t* args, void* stream);

/* ErrorBoundSampler.get_error_bound (reference: model/ray_sampler.py:264-272): z [N,M] sorted, sdf [N,M],
 * dstar [N,M-1], beta [N] (beta_stride 1) or [1] (beta_stride 0) -> out [N] = max opacity error bound per ray. */
int msdf_sampler_error_bound(const float* z, const float* sdf, const float* dstar, const float* beta,
                             int beta_stride, int N, int M, float* out, void* stream);

/* LaplaceDensity.density_func (reference: model/density.py:21-26) on n values laid out in rows of `cols`;
 * beta [1] (beta_stride 0) or one per row (beta_stride 1).  The backward returns d/d sdf and the per-element
 * d/d beta terms (the caller sums them per beta). */
int msdf_laplace_density(const float* sdf, const float* beta, int beta_stride, int64_t n, int cols, float* out,
                         void* stream);
int msdf_laplace_density_backward(const float* sdf, const float* beta, int beta_stride, int64_t n, int cols,
                                  const float* g, float* g_sdf, float* g_beta_elem, void* stream);

/* ---- ray generation (reference: utils/rend_util.py:63-91,105-118 as called at
 * model/network.py:505-516).  uv [n,2] pixel coordinates, pose [4,4] camera-to-world, intrinsics [4,4];
 * outputs: ray_dirs [n,3] world-space unit directions, ray_dirs_cam [n,3] the same ray in the camera frame
 * (the reference's `ray_dirs_tmp`; its z is the depth scale), cam_loc [n,3] the camera centre per ray. */
int msdf_camera_rays(const float* uv, const float* pose, const float* intrinsics, int n, float* ray_dirs,
                     float* ray_dirs_cam, float* cam_loc, void* stream);

/* One pixel-mode training batch assembled on the device (second half; reference: the per-pixel tables of
 * SceneDatasetDN.convert_to_pixels, datasets/scene_dataset.py:269-307, and the pixel branch of __getitem__ 374-401 with
 * the DataLoader's collate + host-to-device copy).  ray_idx [n] int64 in [0, n_frames * hw): ray r is pixel
 * (ray_idx[r] mod hw) of the frame at position ray_idx[r] / hw of frame_list [n_frames] (int32 indices into pose_all /
 * intrinsics_all [N,4,4]; NULL = identity).  The pixel's (u, v) is (column, row) of a row-major image of `width` columns
 * (scene_dataset.py:258-260).  Outputs: ray_dirs, ray_dirs_cam (the reference's ray_dirs_tmp), cam_loc [n,3],
 * ray_pose [n,16], frame_pos [n] int32 (= ray_idx / hw, the reference's ray_frame_idx).  Ground truth: up to 4 image
 * stacks gt_src[k] [n_frames * hw, gt_channels[k]] (rows in frame-list order, device pointers; the arrays of pointers
 * themselves are HOST arrays) gathered into gt_dst[k] [n, gt_channels[k]]; a NULL gt_src[k] is skipped.  An index outside
 * [0, n_frames * hw) touches no memory: its outputs are zeros and its frame_pos is -1. */
int msdf_pixel_rays(const int64_t* ray_idx, int n, const int32_t* frame_list, int n_frames, const float* pose_all,
                    const float* intrinsics_all, int width, int hw, float* ray_dirs, float* ray_dirs_cam,
                    float* cam_loc, float* ray_pose, int32_t* frame_pos, const float* const* gt_src,
                    float* const* gt_dst, const int32_t* gt_channels, int n_gt, void* stream);

/* ---- marching cubes (csrc/mcubes.hip; reference: skimage.measure.marching_cubes at utils/plots.py:199-205).
 * vol: fp32 [nx, ny, nz] in C order (axis 0 = x), every dim >= 2, nx * ny * nz < 2^31.  Corners with v < level are
 * below, the rest above; the case table is csrc/mc_tables.h (generated by scripts/gen_mc_tables.py).
 * msdf_mc_count: classifies every cell into the caller's DEVICE workspace (msdf_mc_workspace_bytes() bytes, 16-byte
 * aligned; -1 for dims out of range) and writes totals[0] = vertices V, totals[1] = triangles F (int64, device).
 * msdf_mc_emit: with the workspace of a count call on the same volume and level, and V, F < 2^31: verts [V,3]
 * (idx + t e_a) * spacing, normals [V,3] (the central-difference gradient interpolated along the edge, normalised;
 * zero gradient -> 0), faces [F,3] int32 oriented by the right-hand rule from below toward above.  Vertices are
 * ordered by (linear voxel index, edge axis), faces by (linear cell index, table order): no atomics, the outputs are
 * bitwise identical run to run. */
int64_t msdf_mc_workspace_bytes(int nx, int ny, int nz);
int msdf_mc_count(const float* vol, int nx, int ny, int nz, float level, void* workspace, int64_t* totals,
                  void* stream);
int msdf_mc_emit(const float* vol, int nx, int ny, int nz, float level, float sx, float sy, float sz,
                 const void* workspace, float* verts, float* normals, int32_t* faces, void* stream);

/* ---- mesh evaluation (csrc/nnsearch.hip): exact nearest neighbours and the voxel down-sample.
 * msdf_nn_search: for every query[i] (fp32 xyz, [n_query, 3]) the index idx[i] (int32) and the Euclidean distance
 * dist[i] of the closest point of ref ([n_ref, 3] fp32), by brute force.  The squared distance is
 * dx dx + dy dy + dz dz from the three differences, in fp32.  Of several reference points at the same fp32 squared
 * distance the smallest index wins; outputs are bitwise the same on every call and for every split count.
 * 1 <= n_ref < 2^31 (0 is an argument error), 0 <= n_query < 2^31 (0 launches nothing).  All coordinates must be
 * finite: the result is undefined otherwise.  n_splits: over how many slices of the reference cloud the work is
 * spread (partial minima merged by a second kernel); <= 0 lets the library choose from the sizes, a positive value is
 * clamped to the number of 1024-point tiles.  msdf_nn_split_count returns the count actually used (-1 for sizes out of
 * range).  workspace: DEVICE, msdf_nn_workspace_bytes(n_ref, n_query, n_splits) bytes for the same three values
 * (-1 for sizes out of range), 8-byte aligned; contents are scratch.
 * msdf_voxel_keys: keys[i] (int64) = (ix << 42) | (iy << 21) | iz of points[i] ([n, 3] fp32), with
 * i* = floor((p - (min_bound - voxel_size / 2)) / voxel_size) per axis, every operation rounded separately in fp32;
 * min_bound: 3 floats on the DEVICE, the per-axis minimum of the cloud.  The caller guarantees every coordinate index
 * < 2^21 (larger ones are clamped).  voxel_size > 0.
 * msdf_voxel_mean: with order[n] (int64) the permutation of a STABLE sort of the keys and seg_start[m] (int64) the
 * positions in the sorted sequence where a new key begins: out[s] ([m, 3] fp32) = the mean of the points of voxel s,
 * their fp64 sum in ascending original index over their count, rounded once to fp32.  No atomics. */
int msdf_nn_split_count(int64_t n_ref, int64_t n_query, int n_splits);
int64_t msdf_nn_workspace_bytes(int64_t n_ref, int64_t n_query, int n_splits);
int msdf_nn_search(const float* ref, int64_t n_ref, const float* query, int64_t n_query, int n_splits,
                   void* workspace, float* dist, int32_t* idx, void* stream);
int msdf_voxel_keys(const float* points, int64_t n, const float* min_bound, float voxel_size, int64_t* keys,
                    void* stream);
int msdf_voxel_mean(const float* points, const int64_t* order, const int64_t* seg_start, int64_t n, int64_t m,
                    float* out, void* stream);

/* ---- mesh re-fusion (csrc/refuse.hip; reference: scannet_eval/evaluate.py:111-137, postprocess/refuse.py,
 * replica_eval/cull_mesh.py:58-87).  Cameras are OpenCV-style (x right, y down, z forward).  w2c: [n_views, 12] fp32 on
 * the DEVICE, the first three rows of the world-to-camera matrix of every view, row-major (r00 r01 r02 tx ...).
 * No floating-point atomics anywhere: outputs are bitwise identical run to run.
 * msdf_raster_depth: depth [n_views, height, width] fp32 = camera-frame z of the nearest intersection of the ray through
 * ((j + pixel_center - cx) / fx, (i + pixel_center - cy) / fy, 1) with any face (both windings) of the mesh verts
 * [n_verts, 3] fp32 (world) / faces [n_faces, 3] int32, among intersections with znear <= z <= zfar; 0 where there is
 * none.  Two faces that share an edge leave no crack between them.  A face with an index outside [0, n_verts) or
 * without area touches no pixel; n_faces = 0 gives zeros.  0 < znear <= zfar, n_views <= 65535, height * width < 2^31.
 * msdf_tsdf_integrate: a dense block of nx x ny x nz voxels (C order, < 2^31), voxel (i, j, k) centred at
 * o + voxel_length (i + i0 + 0.5, j + j0 + 0.5, k + k0 + 0.5) ((i0, j0, k0) >= 0: where the block starts in a larger
 * volume with origin o; index + offset < 2^24, exact in fp32, so a voxel that two blocks share has the same centre
 * in both), fused from the depth maps [n_views, height, width] in the order given
 * by the rule of open3d's UniformTSDFVolume (separately rounded fp32 operations): p = R x + t, skipped unless p.z > 0;
 * u = int(fx p.x / p.z + cx + 0.5), v likewise, skipped outside the image; d = depth[v, u], skipped unless
 * 0 < d <= depth_trunc; s = (d - p.z) |((u - cx) / fx, (v - cy) / fy, 1)|, skipped if s <= -sdf_trunc;
 * tsdf = (tsdf w + min(1, s / sdf_trunc)) / (w + 1), w += 1, from tsdf = w = 0 (resume = 0) or from what tsdf and
 * weight hold (resume = 1: a further chunk of the same list of views).  Outputs tsdf, weight [nx, ny, nz].
 * msdf_tsdf_face_keep: keep[f] (uint8) = 1 iff every lattice point in [floor(min), ceil(max)] per axis of the three
 * vertices of face f (verts in index units, as marching cubes gives them with spacing 1) has weight > 0; 0 for a face
 * with a vertex outside the lattice or an index outside [0, n_verts).
 * msdf_cull_vertices: seen[i] (uint8) = 1 iff for some view, with p = R x + t: p.z >= 1e-5 and
 * 0 < fx p.x / (p.z - 1e-5) + cx < width and 0 < fy p.y / (p.z - 1e-5) + cy < height (separately rounded fp32). */
int msdf_raster_depth(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* w2c,
                      int n_views, float fx, float fy, float cx, float cy, int height, int width, float znear,
                      float zfar, float pixel_center, float* depth, void* stream);
int msdf_tsdf_integrate(const float* depth, const float* w2c, int n_views, float fx, float fy, float cx, float cy,
                        int height, int width, float ox, float oy, float oz, int i0, int j0, int k0, int nx, int ny,
                        int nz, float voxel_length, float sdf_trunc, float depth_trunc, int resume, float* tsdf,
                        float* weight, void* stream);
int msdf_tsdf_face_keep(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                        const float* weight, int nx, int ny, int nz, uint8_t* keep, void* stream);
int msdf_cull_vertices(const float* verts, int64_t n_verts, const float* w2c, int n_views, float fx, float fy, float cx,
                       float cy, int height, int width, uint8_t* seen, void* stream);

/* ---- the DTU evaluation protocol (csrc/dtueval.hip; reference: dtu_eval/evaluate_single_scene.py:20-103 and
 * dtu_eval/eval.py:43-134).  Integer, boolean, separately rounded fp32 or fp64 rules only and no floating-point
 * atomics: outputs are bitwise identical run to run.  All buffers are the caller's, on the DEVICE unless said.
 * msdf_dtu_dilate: out [n_views, height, width] uint8 (0 / 1) = the views of masks (uint8, set iff non-zero) dilated by
 * skimage's disk(radius), the offsets with dx^2 + dy^2 <= radius^2; pixels outside the image are unset.
 * 0 <= radius <= 32, n_views * height * width <= 2^37.  workspace: msdf_dtu_dilate_workspace_bytes() bytes (-1 for
 * sizes out of range), 4-byte aligned, scratch.
 * msdf_dtu_mask_vertices: keep[i] (uint8) = 1 iff in every view v, with P = proj[v] ([n_views, 12] fp32, rows of the
 * 3x4 projection whose third row gives camera depth) and separately rounded fp32 operations:
 * (u, v, z) = ((P0 x + P1 y) + P2 z) + P3 per row, px = u / (z + 1e-6), py = v / (z + 1e-6), the vertex is not valid
 * (valid: 0 < px < width - 1 and 0 < py < height - 1) or dilated[v, rint(py), rint(px)] != 0 (half to even).  There is
 * no test of the sign of z.  n_views = 0 keeps every vertex.
 * msdf_dtu_lattice_count / _emit: the deterministic triangle sampler of eval.py:54-71 in fp64 on the fp32 vertices
 * (verts [n_verts, 3], faces [n_faces, 3] int32; a face with an index outside [0, n_verts) gives nothing):
 * v1 = p1 - p0, v2 = p2 - p0, l = sqrt((x^2 + y^2) + z^2), area2 = |v1 x v2| (a face with area2 == 0 gives nothing),
 * thr = density sqrt(l1 l2 / area2), n = floor(l / thr), candidates a = (i + 0.5) / max(n1, 1e-7), i = 0..n1 and
 * b = (j + 0.5) / max(n2, 1e-7), j = 0..n2, kept iff a + b < 1, point = (v1 a + v2 b) + p0 rounded once to fp32.
 * count writes counts[f] (int64; 2^40 for a face of more than 2^34 candidates, which alone exceeds the limit); emit
 * takes offsets [n_faces + 1] (int64), the exclusive scan of the counts with the total n_points (< 2^31) last, and
 * writes out [n_points, 3] in the order face, i, j.  density > 0.
 * msdf_dtu_thin_*: the greedy radius thinning of eval.py:86-94: visiting the points in order, a point still marked is
 * kept and unmarks every point with ((dx dx + dy dy) + dz dz) <= radius radius (fp64 on the fp32 coordinates).
 *   _keys: keys[i] (int64) = (cx << 42) | (cy << 21) | cz with c = floor((p - lo) / cell) + 1 per axis in fp64,
 *     clamped to [1, 2^21 - 2]; the caller chooses lo <= every coordinate and cell >= radius (1 + 2^-10) with
 *     (max - lo) / cell < 2^21 - 3, so that two points within radius are at most one cell apart.
 *   _prepare: with perm [n] (int64) the permutation of a sort of the keys, sorted_keys [n] the keys in that order and
 *     rank [n] (int64; rank[i] = when point i is visited; NULL = index order): fills the workspace
 *     (msdf_dtu_thin_workspace_bytes(n) bytes, 16-byte aligned) and marks every point undecided.
 *   _round: one round of the iteration (an undecided point with a kept earlier neighbour becomes removed, else with an
 *     undecided one stays, else becomes kept); *undecided (uint32) = how many points remain undecided.  The caller
 *     repeats it until that is 0; the earliest undecided point is decided every round.
 *   _finish: keep[perm[s]] (uint8) = 1 iff the point is kept. */
int64_t msdf_dtu_dilate_workspace_bytes(int n_views, int height, int width);
int msdf_dtu_dilate(const uint8_t* masks, int n_views, int height, int width, int radius, void* workspace,
                    uint8_t* out, void* stream);
int msdf_dtu_mask_vertices(const float* verts, int64_t n_verts, const float* proj, int n_views,
                           const uint8_t* dilated, int height, int width, uint8_t* keep, void* stream);
int msdf_dtu_lattice_count(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                           double density, int64_t* counts, void* stream);
int msdf_dtu_lattice_emit(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, double density,
                          const int64_t* offsets, int64_t n_points, float* out, void* stream);
int64_t msdf_dtu_thin_workspace_bytes(int64_t n);
int msdf_dtu_thin_keys(const float* points, int64_t n, double lo_x, double lo_y, double lo_z, double cell,
                       int64_t* keys, void* stream);
int msdf_dtu_thin_prepare(const float* points, const int64_t* perm, const int64_t* rank, const int64_t* sorted_keys,
                          int64_t n, void* workspace, void* stream);
int msdf_dtu_thin_round(void* workspace, int64_t n, double radius, uint32_t* undecided, void* stream);
int msdf_dtu_thin_finish(const void* workspace, const int64_t* perm, int64_t n, uint8_t* keep, void* stream);

#ifdef __cplusplus
}
#endif
#endif
