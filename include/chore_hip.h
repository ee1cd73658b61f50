/*
 * chore_hip.h -- C ABI of libchore_hip.so, the MI355X (gfx950) implementation of CHORE's
 * implicit-field query + fitting hot path.
 *
 * The reference (xiexh20/CHORE) has no FFI seam of its own for this path: the hot path is pure
 * ATen called from Python (model/chore.py:87-167).  The only C boundary in the reference tree is
 * the vendored rasterizer's pybind module (external/neural_renderer/neural_renderer/cuda/
 * rasterize_cuda.cpp:201-207), whose conventions we mirror: the CALLER allocates every buffer
 * (inputs, outputs, workspaces), functions fill them and return; work is enqueued on the caller's
 * stream; no hidden synchronisation, no internal threads.  Each entry point below cites the
 * reference code it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless stated otherwise
 *   - return 0 (CHORE_OK) on success, negative CHORE_E* otherwise; chore_last_error() gives text
 *   - `stream` is a hipStream_t passed as void*; NULL = the default stream
 *   - nothing here calls hipMalloc/hipFree/hipDeviceSynchronize on the hot path, so every call is
 *     hipGraph-capturable
 *   - one handle per (process, device); a handle is not thread-safe
 */
#ifndef CHORE_HIP_H
#define CHORE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct chore_handle chore_handle;
typedef void* chore_stream_t;

enum {
    CHORE_OK = 0,
    CHORE_EINVAL = -1, /* bad argument (shape, dtype, null pointer)   */
    CHORE_EHIP = -2,   /* a HIP runtime call failed                    */
    CHORE_ESTATE = -3, /* missing weights / wrong call order           */
    CHORE_ENOMEM = -4  /* caller workspace too small                   */
};

/* storage / MFMA-operand type of feature maps and packed weights */
enum { CHORE_F32 = 0, CHORE_BF16 = 1, CHORE_F16X3 = 2, CHORE_F16 = 3 };
/* CHORE_F16 ("fp16 fields", inference only): IEEE half feature maps; the encoder's convolutions multiply the fp16 activation
 * by the weight's fp16 hi and lo parts (two MFMAs per product, fp32 accumulation); the heads run as under CHORE_HEADS_X3. */
/* query entry points (chore_query_fwd / _bwd_points / _fwd_train / _bwd_train, chore_heads_wgrad): OR into the map type
 * to run the MLP heads on the fp16 matrix cores with hi/lo split operands (fp32-grade results, see csrc/heads_x3.h)
 * instead of the native fp32 MFMA.  CHORE_F16X3 there means CHORE_F32 | CHORE_HEADS_X3. */
enum { CHORE_HEADS_X3 = 0x100 };

/* one tensor of a reference state_dict (Appendix D of SURVEY.md): name, device pointer to its
 * contiguous fp32 data in the reference layout, element count */
typedef struct {
    const char* name;
    const void* ptr;
    int64_t numel;
} chore_weight_desc;

/* encoder topology = the fields of config/chore-release.json the hot path reads
 * (model/HGFilters.py:57-142) */
typedef struct {
    int in_channels;   /* 5 for input_type RGBM3                         */
    int num_stack;     /* 5                                              */
    int num_hourglass; /* 2 (recursion depth of one hourglass)           */
    int hourglass_dim; /* 256                                            */
} chore_encoder_cfg;

int chore_version(void);
int chore_create(chore_handle** out, int device_ordinal);
int chore_destroy(chore_handle* h);
const char* chore_last_error(const chore_handle* h);

/* Streams restricted to a subset of the compute units (no reference counterpart: the reference's loader loop,
 * recon/recon_fit_behave.py:41-76, is serial; this serves the pipelined loop of ReconFitterBehave.fit_recon, where the
 * preparation of batch k+1 must leave CUs free for the small kernels of batch k's optimisation).
 * mask: n_words x 32 bits, bit i = one CU (dealt round robin over the XCDs); chore_cu_count = CUs of the handle's device.
 * The stream is a plain hipStream_t: hand it to any entry point, destroy it with chore_stream_destroy (waits for it). */
int chore_cu_count(chore_handle* h);
int chore_stream_create_cu_mask(chore_handle* h, const uint32_t* mask, int n_words, chore_stream_t* out);
int chore_stream_destroy(chore_handle* h, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-point MLP heads + fused query  (replaces CHORE.query, model/chore.py:107-154:
 * camera.project_points model/camera.py:44-88, index()/grid_sample model/geometry.py:4-14 twice,
 * torch.cat, CHORE.decode model/chore.py:156-167, the df[~in_img]=OUT_DIST fill :147-150)
 * ------------------------------------------------------------------------------------------- */

/* bytes of the packed (MFMA-fragment-ordered) weight arena of the four heads */
size_t chore_heads_arena_bytes(int dtype);

/* Repack the four decoders' Conv1d weights into the arena.  `descs` must contain
 * {df,part_predictor,pca_predictor,center_predictor}.{0,2,4,6}.{weight,bias} (fp32, reference
 * layout (out,in,1)).  model/chore.py:49-55,74-85. */
int chore_heads_pack(chore_handle* h, const chore_weight_desc* descs, int n_descs, int dtype,
                     void* arena, chore_stream_t stream);

/* Camera constants in the order (fx_px, fy_px, cx_px, cy_px, crop/2, crop) -- HOST pointer to 6
 * floats, values as computed in model/camera.py:26-42. */

/* Fused forward query.
 *   points      (B,N,3) fp32 camera-space      crop_center (B,2) fp32
 *   feat        (B,FH,FW,256) NHWC `dtype`     tmpx (B,TH,TW,64) NHWC `dtype`
 *   df (B,2,N)  pca (B,9,N)  parts (B,14,N)  centers (B,6,N)  fp32;  in_img (B,N) uint8 (may be NULL)
 * df is written with OUT_DIST (5.0) where the projected point falls outside [-1,1]^2.
 * Any of df / pca / parts / centers may be NULL (not all four): that head is not evaluated (its wave leaves after the
 * gather).  chore_query_bwd_points skips the chain of every head whose upstream gradient is NULL. */
int chore_query_fwd(chore_handle* h, const float* points, const float* crop_center, int B, int N,
                    const void* feat, int FH, int FW, const void* tmpx, int TH, int TW, int dtype,
                    const void* heads_arena, const float* cam6_host, float* df, float* pca,
                    float* parts, float* centers, uint8_t* in_img, chore_stream_t stream);

/* chore_query_fwd in SORTED ORDER: with a workspace of chore_query_fwd_workspace_bytes(B, N) bytes (NULL = chore_query_fwd) the points of
 * a large query with the fp16 x 3 heads are first ordered by the 8 x 8-texel tile of the feature map their sample falls into (two
 * small launches writing a permutation into the workspace) and the tiles of 64 points are formed in that order, so that a tile's
 * gather (BasePIFuNet.index, model/geometry.py:4-14, called from model/chore.py:134-143) reads a texel row once instead of once per
 * point: a third of the fetched bytes.  Every point's arithmetic is unchanged and its outputs go to its own column: results are
 * bit-identical to chore_query_fwd's.  The two extra launches cost more time than the gather saves on one MI355X (DESIGN.md section
 * 4): the host code passes a workspace only with CHORE_QUERY_SORTED=1.  Shapes the ordering does not cover (fewer than 8 192 points,
 * feature maps of more than 256 tiles, the native-fp32 heads) run exactly as chore_query_fwd. */
size_t chore_query_fwd_workspace_bytes(int B, int N);
int chore_query_fwd_ws(chore_handle* h, const float* points, const float* crop_center, int B, int N,
                       const void* feat, int FH, int FW, const void* tmpx, int TH, int TW, int dtype,
                       const void* heads_arena, const float* cam6_host, float* df, float* pca,
                       float* parts, float* centers, uint8_t* in_img, void* workspace, chore_stream_t stream);

/* Pixel-aligned feature sample without the heads: BasePIFuNet.index (model/BasePIFuNet.py:23 ->
 * model/geometry.py:4-14) on both maps plus z_feat, concatenated as in model/chore.py:139-143.
 *   features (B,N,323) fp32 point-major [feat 0..255 | x y z-2.2 | tmpx 0..63]
 *   nxy (B,N,2) normalised image coordinates of model/camera.py:44-88 (may be NULL)
 *   in_img (B,N) uint8 (may be NULL) */
int chore_sample_features(chore_handle* h, const float* points, const float* crop_center, int B, int N,
                          const void* feat, int FH, int FW, const void* tmpx, int TH, int TW, int dtype,
                          const float* cam6_host, float* features, float* nxy, uint8_t* in_img,
                          chore_stream_t stream);

/* Backward of chore_query_fwd with respect to the POINTS only (what
 * recon/generator.py:62-77 `df_target.sum().backward()` and every fitting loss need):
 * g_* are the upstream gradients of the four outputs (any may be NULL = zero); the forward is
 * recomputed inside the kernel, nothing is saved.  Gradients of df at out-of-image points are
 * dropped (the in-place fill of model/chore.py:149 cuts the graph there).
 *   dpoints (B,N,3) fp32, overwritten. */
int chore_query_bwd_points(chore_handle* h, const float* points, const float* crop_center, int B,
                           int N, const void* feat, int FH, int FW, const void* tmpx, int TH,
                           int TW, int dtype, const void* heads_arena, const float* cam6_host,
                           const float* g_df, const float* g_pca, const float* g_parts,
                           const float* g_centers, float* dpoints, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training backward of the query (first half of the backward of CHORE.forward, model/chore.py:176-190: what the
 * reference's autograd computes for Trainer.train_step, trainer/trainer.py:76-131, through decode :156-167 and
 * index / grid_sample model/geometry.py:4-14).  chore_query_bwd_train recomputes the forward like
 * chore_query_bwd_points and, besides dpoints (optional), stages in `staging` (chore_query_train_bytes):
 *   X   [B*N][328]          the 323-vector of every point, zero padded
 *   H   [3][4][B*N][128]    relu outputs of hidden layers 1..3, heads in the order df, parts, pca, centers
 *   dZ  [3][4][B*N][128]    gradients w.r.t. the pre-activations of layers 1..3
 *   dX  [B*N][328]          gradient w.r.t. the 323-vector, summed over the heads
 * chore_heads_wgrad turns the staging into the gradients of all 32 head parameters (dW_l = dZ_l^T H_{l-1}, db_l = column
 * sums of dZ_l; the output layers use the upstream gradients directly -- pass g_df already zeroed where the point is
 * outside the image, model/chore.py:147-150): `grads` = chore_heads_wgrad_floats() floats, per head in kernel order
 * (df, parts, pca, centers): W1 (128,323) b1 (128) W2 (128,128) b2 W3 b3 W4 (out,128) b4 (out); ordered partial sums,
 * bit-reproducible.  workspace: chore_heads_wgrad_workspace_bytes().
 * chore_scatter_features turns dX into the gradients of the two feature maps: dfeat (B,FH,FW,256) and dtmpx
 * (B,TH,TW,64), fp32 NHWC, written (accumulate = 0) or added to (accumulate = 1); tile-gather, no atomics.
 * ------------------------------------------------------------------------------------------- */
size_t chore_query_train_bytes(int B, int N);
/* training forward: chore_query_fwd that also stages the 323-vectors and the ReLU outputs (X, H of the layout above) */
int chore_query_fwd_train(chore_handle* h, const float* points, const float* crop_center, int B, int N,
                          const void* feat, int FH, int FW, const void* tmpx, int TH, int TW, int map_dtype,
                          const void* heads_arena, const float* camera, float* df, float* pca, float* parts,
                          float* centers, uint8_t* in_img, void* staging, chore_stream_t stream);
/* have_forward != 0: `staging` already holds X and H from chore_query_fwd_train of the same inputs; the backward
 * then recomputes nothing (ReLU masks are read back) and only adds dZ and dX */
int chore_query_bwd_train(chore_handle* h, const float* points, const float* crop_center, int B, int N,
                          const void* feat, int FH, int FW, const void* tmpx, int TH, int TW, int map_dtype,
                          const void* heads_arena, const float* camera, const float* g_df, const float* g_pca,
                          const float* g_parts, const float* g_centers, void* staging, float* dpoints,
                          int have_forward, chore_stream_t stream);
size_t chore_heads_wgrad_floats(void);
size_t chore_heads_wgrad_workspace_bytes(void);
int chore_heads_wgrad(chore_handle* h, const void* staging, int B, int N, const float* g_df, const float* g_pca,
                      const float* g_parts, const float* g_centers, float* grads, void* workspace,
                      int heads_x3 /* bit 0: fp16 matrix cores, split operands, per-chunk scales (see CHORE_HEADS_X3); bit 1: add to
                                      `grads` instead of overwriting (the stacks of a step into one arena) */,
                      chore_stream_t stream);
int chore_scatter_features(chore_handle* h, const float* points, const float* crop_center, int B, int N, int FH, int FW,
                           int TH, int TW, const float* camera, const void* staging, float* dfeat, float* dtmpx,
                           int accumulate, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Stacked-hourglass encoder  (replaces HGFilter.forward model/HGFilters.py:144-185,
 * HourGlass._forward :26-50, ConvBlock.forward model/net_util.py:374-396)
 * ------------------------------------------------------------------------------------------- */

/* bytes of the packed encoder weight arena */
size_t chore_encoder_arena_bytes(const chore_encoder_cfg* cfg, int dtype);

/* Repack `image_filter.*` tensors of the state_dict (fp32, reference layouts) into the arena. */
int chore_encoder_pack(chore_handle* h, const chore_encoder_cfg* cfg,
                       const chore_weight_desc* descs, int n_descs, int dtype, void* arena,
                       chore_stream_t stream);

/* caller-allocated scratch needed by chore_encode_fwd for this shape */
size_t chore_encoder_workspace_bytes(const chore_encoder_cfg* cfg, int B, int H, int W, int dtype);

/* images (B,C,H,W) fp32 NCHW in [0,1] as data/test_data.py:107-125 delivers them.
 * feat_out[i] (B,H/4,W/4,256) NHWC `dtype` for the last `n_stack_out` stacks (eval: 1, training:
 * num_stack; model/chore.py:93-96), tmpx (B,H/2,W/2,64), normx (B,H/4,W/4,128) (may be NULL). */
int chore_encode_fwd(chore_handle* h, const chore_encoder_cfg* cfg, const float* images, int B,
                     int H, int W, int dtype, const void* arena, void* workspace,
                     size_t workspace_bytes, void* const* feat_out, int n_stack_out, void* tmpx,
                     void* normx, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SMPL / SMPL-H linear blend skinning  (replaces SMPL_Layer.forward,
 * lib_smpl/smplpytorch/smplpytorch/pytorch/smpl_layer.py:72-175 -- batch_rodrigues
 * rodrigues_layer.py:41-52, th_posemap_axisang / subtract_flat_id tensutils.py:6-53 -- and its
 * autograd w.r.t. pose, betas and trans, which is what recon/recon_fit_behave.py:224-291 optimises)
 *   model buffers (fp32, reference layouts): v_template (V,3), shapedirs (V,3,num_betas),
 *   posedirs (V,3,9(J-1)), J_regressor (J,V) dense, weights (V,J); parents: HOST array of J ints
 *   (kintree_table[0]; parents[0] ignored, parents[i] < i).
 * ------------------------------------------------------------------------------------------- */
size_t chore_smpl_arena_bytes(int V, int J, int num_betas);
size_t chore_smpl_workspace_bytes(int V, int J, int num_betas, int B);
int chore_smpl_pack(chore_handle* h, int V, int J, int num_betas, const float* v_template,
                    const float* shapedirs, const float* posedirs, const float* J_regressor,
                    const float* weights, const int* parents_host, void* arena, chore_stream_t stream);
/* pose (B,3J) axis-angle, betas (B,num_betas), trans (B,3), offsets (B,V,3) or NULL ->
 * verts (B,V,3), joints (B,J,3), v_posed (B,V,3), naked (B,V,3).  `workspace` must be kept untouched
 * until the matching chore_smpl_lbs_bwd call (it holds the rotations / transforms of this call). */
int chore_smpl_lbs_fwd(chore_handle* h, const void* arena, int V, int J, int num_betas, const float* pose,
                       const float* betas, const float* trans, const float* offsets, float scale, int B,
                       float* verts, float* joints, float* v_posed, float* naked, void* workspace,
                       chore_stream_t stream);
/* g_verts (B,V,3) / g_joints (B,J,3) upstream gradients (either may be NULL) ->
 * dpose (B,3J), dbetas (B,num_betas), dtrans (B,3) */
int chore_smpl_lbs_bwd(chore_handle* h, const void* arena, int V, int J, int num_betas, const float* pose,
                       float scale, int B, const float* v_posed, const float* g_verts, const float* g_joints,
                       float* dpose, float* dbetas, float* dtrans, void* workspace, chore_stream_t stream);
/* landmark regression on the skinned vertices (replaces the per-regressor torch.sparse.mm loop of
 * lib_smpl/torch_functions.py:52-76 behind SMPLPyTorchWrapperBatch.get_landmarks, lib_smpl/wrapper_pytorch.py:186-205):
 * reg (R,V) dense fp32 (rows of the body-25 / face / hand regressors stacked), verts (B,V,3) -> out (B,R,3); backward:
 * g (B,R,3) -> dverts (B,V,3), written (not accumulated); R <= 2048 */
int chore_landmarks_fwd(chore_handle* h, const float* reg, const float* verts, int R, int V, int B, float* out,
                        chore_stream_t stream);
int chore_landmarks_bwd(chore_handle* h, const float* reg, const float* g, int R, int V, int B, float* dverts,
                        chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Projection onto SO(3)  (replaces ReconFitterBase.project_so3, recon/recon_fit_base.py:168-188:
 * R = U diag(1,1,det(UV^T)) V^T) and its backward.  M, R, G, dM are (B,3,3) fp32 row-major;
 * `aux` (chore_so3_aux_bytes(B) bytes, may be NULL if no backward follows) carries U, V, sigma.
 * ------------------------------------------------------------------------------------------- */
size_t chore_so3_aux_bytes(int B);
int chore_so3_project_fwd(chore_handle* h, const float* M, int B, float* R, void* aux, chore_stream_t stream);
int chore_so3_project_bwd(chore_handle* h, const void* aux, const float* G, int B, float* dM,
                          chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Human-object contact term of the joint fitting phase  (replaces ReconFitterBase.compute_contact_loss,
 * recon/recon_fit_base.py:553-608, and the pytorch3d.loss.chamfer_distance call at :605-607 with its
 * defaults: squared-L2 nearest neighbour, mean over the points of a cloud, mean over clouds, both
 * directions added).  hum (B,Nh,3), obj (B,No,3); df_hum_o (B,Nh) = object distance field at the human
 * vertices, df_obj_h (B,No) = human distance field at the object points (contact = value < thres);
 * label_h (Nh) int32 part label of every human vertex; part_logits (B,P,No) object part logits (argmax
 * inside).  loss: 1 float on the device (0 when no (frame, part) pair has contact points on both sides).
 * `workspace` (chore_contact_workspace_bytes) carries the nearest-neighbour indices to the backward.
 * No host synchronisation: the step can be captured in a hipGraph.
 * ------------------------------------------------------------------------------------------- */
size_t chore_contact_workspace_bytes(int B, int Nh, int No, int P);
int chore_contact_fwd(chore_handle* h, const float* hum, const float* obj, const float* df_hum_o,
                      const float* df_obj_h, const int* label_h, const float* part_logits, int B, int Nh, int No,
                      int P, float thres, float* loss, void* workspace, chore_stream_t stream);
/* g_loss: 1 float on the device (upstream gradient) -> d_hum (B,Nh,3), d_obj (B,No,3); one of the two may be NULL (not
 * computed) */
int chore_contact_bwd(chore_handle* h, const float* hum, const float* obj, const int* label_h, int B, int Nh,
                      int No, int P, const float* g_loss, const void* workspace, float* d_hum, float* d_obj,
                      chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Differentiable silhouette rasterisation for the mask loss of the object fit  (replaces neural_renderer's
 * RasterizeFunction with return_alpha only, external/neural_renderer/neural_renderer/rasterize.py:14-170, i.e.
 * the CUDA kernels forward_face_index_map cuda/rasterize_cuda_kernel.cu:24-215 and backward_pixel_map
 * :290-549, as used by SilLossROI.forward recon/obj_pose_roi.py:159-172).
 * faces (B,F,3,3) fp32: projected triangle vertices [u, v in [-1,1], depth] (after fill_back, i.e. both windings);
 * face_index (B,size,size) int32 (-1 = background), alpha (B,size,size) fp32 in {0,1}; rows are NOT flipped
 * (the caller flips like rasterize_rgbad does, rasterize.py:345).  near/far/eps defaults of the reference:
 * 0.1, 100, 1e-4.  No face is dropped (the reference keeps at most 512 per 4x4-pixel block) and equal depths
 * resolve to the smaller face index.
 * ------------------------------------------------------------------------------------------- */
size_t chore_silhouette_workspace_bytes(int B, int F);
int chore_silhouette_fwd(chore_handle* h, const float* faces, int B, int F, int size, float near_z, float far_z,
                         int* face_index, float* alpha, void* workspace, chore_stream_t stream);
/* grad_alpha (B,size,size) -> grad_faces (B,F,3,3) (depth components are zero) */
int chore_silhouette_bwd(chore_handle* h, const float* faces, const int* face_index, const float* alpha,
                         const float* grad_alpha, int B, int F, int size, float eps, float* grad_faces,
                         chore_stream_t stream);
/* The rasteriser's triangle list from the object pose in one launch: SilLossROI.apply_transformation (recon/obj_pose_roi.py:
 * 159-162, w = s (v Ro + to)), neural_renderer's projection (external/neural_renderer/neural_renderer/projection.py:6-43:
 * c = Rc w + tc, divide by z + eps, distortion polynomial, K, [-1,1] with the vertical flip) and vertices_to_faces with both
 * windings (renderer.py:119-152, fill_back).  verts (B,V,3) template, faces (B,F,3) int32, obj_R (B,3,3) applied as v Ro,
 * obj_t (B,3), obj_s (B), K (B,3,3), cam_R / cam_t (B,3,3) / (B,3) or one for all frames (cam_broadcast != 0), dist5 HOST
 * {k1,k2,p1,p2,k3} or NULL -> tri (B,2F,3,3): face f and, at F + f, its reversed winding.
 * Backward: g_tri (B,2F,3,3) -> d_obj_R, d_obj_t, d_obj_s; adj_off (V+1) / adj: for every vertex the entries (f2 * 3 + corner)
 * of the doubled list that reference it, ascending (the order its corner gradients are added in; one topology for all frames). */
int chore_sil_project_fwd(chore_handle* h, const float* verts, const int* faces, const float* obj_R, const float* obj_t,
                          const float* obj_s, const float* K, const float* cam_R, const float* cam_t, int cam_broadcast,
                          const float* dist5, float orig_size, float eps, int B, int V, int F, float* tri,
                          chore_stream_t stream);
int chore_sil_project_bwd(chore_handle* h, const float* verts, const float* obj_R, const float* obj_t, const float* obj_s,
                          const float* K, const float* cam_R, const float* cam_t, int cam_broadcast, const float* dist5,
                          float orig_size, float eps, int B, int V, int F, const int* adj_off, const int* adj,
                          const float* g_tri, float* d_obj_R, float* d_obj_t, float* d_obj_s, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The silhouette term's targets on the device, and PHOSA's edge term  (replaces the host work of SilLossROI's constructor,
 * recon/obj_pose_roi.py:21-103,125-157: np.nonzero boxes, one grid_sample per frame, scipy's distance_transform_edt per frame).
 * Every call is a fixed sequence of launches on `stream`, reads no device value on the host and allocates nothing: it can be
 * captured into a graph.  Fills are kernels, atomics are integer only, float sums have a fixed order: same inputs, same bits.
 *
 * chore_edt_sq: feature (B,H,W) bytes -> d2 (B,H,W) int32, the exact squared Euclidean distance from every pixel to the
 * nearest pixel of the same image whose feature byte is non-zero (integers throughout).  H, W <= 4096 (d2 < 2^25), anything
 * larger is CHORE_EINVAL.  An image WITHOUT any feature pixel gets the sentinel 2 * max(H,W)^2 everywhere (larger than any real
 * value; what scipy returns in that case is an artefact of its implementation and is not reproduced).  workspace:
 * chore_edt_workspace_bytes (0 = unsupported shape).  chore_edt_sqrt_f64: out[i] = sqrt((double) d2[i]), correctly rounded.
 * chore_edt_tiles: the column pass's columns per block, the row pass's threads per block, the largest H / W (host; for tests).
 * ------------------------------------------------------------------------------------------- */
size_t chore_edt_workspace_bytes(int B, int H, int W);
int chore_edt_sq(chore_handle* h, const uint8_t* feature, int B, int H, int W, int* d2, void* workspace, chore_stream_t stream);
int chore_edt_sqrt_f64(chore_handle* h, const int* d2, size_t n, double* out, chore_stream_t stream);
int chore_edt_tiles(int* col_tile, int* row_tile, int* max_dim);
/* What compute_edges and prepare_dist_trans produce from image_ref (B,S,S): edges = maxpool_k(image_ref) - image_ref (stride 1,
 * padding k/2 that never wins, k odd <= 31) and edt = (float) sqrt(sqrt((double) d2)) for power == 0.25, in general
 * (float) pow(sqrt((double) d2), 2 power), d2 = chore_edt_sq of the feature edges > 0 (its sentinel for a frame without edges). */
size_t chore_sil_edge_edt_workspace_bytes(int B, int S);
int chore_sil_edge_edt(chore_handle* h, const float* image_ref, int B, int S, int ksize, float power, float* edges, float* edt,
                       void* workspace, chore_stream_t stream);
/* person, obj (B,H,W) masks, crop_centers (B,2) ->
 *   box_sq (B,4) double: make_bbox_square(xywh box of obj > 0.5, expansion) as x, y, s, s;  valid (B) int32: 1 if obj > 0.5 anywhere;
 *   K (B,3,3): compute_K_roi(to_original_bbox(box_sq, crop_size / net_input_size, crop_center, crop_size)), computed in double
 *     in the operation order of the Python functions, each operation rounded once, rounded to float at the end;
 *   image_ref, keep_mask (B,S,S): the bilinear crops of obj / person over box_sq sampled at the output grid's pixel centres
 *     x + (i + 0.5) s / S - 0.5 (coordinates and weights in double, zeros outside), thresholded at >= 0.5, then
 *     image_ref = obj crop, keep_mask = obj crop or not person crop (cvt_masks).
 * A frame whose object mask is empty gets valid = 0, all-zero image_ref and keep_mask (its mask term is 0) and the K of the
 * box (0, 0, max(H,W), max(H,W)). */
size_t chore_sil_targets_workspace_bytes(int B);
int chore_sil_targets(chore_handle* h, const float* person, const float* obj, const float* crop_centers, int B, int H, int W,
                      int S, double expansion, double crop_size, int net_input_size, float* image_ref, float* keep_mask, float* K,
                      double* box_sq, int* valid, void* workspace, chore_stream_t stream);
/* per_frame_sum[b] = sum_pixels (maxpool_k(image) - image) * weight, image / weight (B,S,S); argmax (B,S,S) int32 = y * S + x of
 * the window's first maximum in row-major order (torch.max_pool2d's rule; NaN inputs are out of scope).  The sum is a tree over
 * blocks of 256 pixels (8 additions deep), then per frame thread t adds block sums t, t + 256, ... and the same tree follows:
 * the longest chain is 16 + ceil(ceil(S^2 / 256) / 256) additions.  workspace: chore_sil_edge_workspace_bytes.
 * Backward, gather form: g_image[p] = g_per_frame[b] * (sum_{q: argmax[q] == p} weight[q] - weight[p]), q in row-major order. */
size_t chore_sil_edge_workspace_bytes(int B, int S);
int chore_sil_edge_fwd(chore_handle* h, const float* image, const float* weight, int B, int S, int ksize, float* per_frame_sum,
                       int* argmax, void* workspace, chore_stream_t stream);
int chore_sil_edge_bwd(chore_handle* h, const float* weight, const int* argmax, const float* g_per_frame, int B, int S, int ksize,
                       float* g_image, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * PHOSA's ordinal depth term for the object fit: the masks say who is in front  (not in the reference's fit; PHOSA's
 * losses.py compute_ordinal_depth_loss is the model).  On the S x S grid of the silhouette term, per frame:
 *   d_o(p)  depth of the object face that wins pixel p: the face chore_silhouette_fwd writes for the step's triangle list
 *           `tri` (B,F,3,3), and zp of the depth rule of chore_render_fwd (clamped, renormalised barycentric weights from the
 *           pixel-space inverse, 1 / sum w_k / z_k) -- the value chore_render_fwd writes at ssaa 1, bit for bit;
 *   d_h(p)  occluder_depth (B,S,S): the same quantity of the body, far_z where there is no body; a constant, no gradient;
 *   both    an object face won (face_index in [0, F)) and d_h < far_z;
 *   O = image_ref > 0.5 (the object), P = not O and keep_mask < 0.5 (the person without the object: a pixel the crops label
 *           both ways counts as object, as for the mask term -- the one difference from PHOSA's mask_i & ~mask_j);
 *   case A  P and both and d_o < d_h: x = min(d_h - d_o, c), term log1p(exp(x)), d term / d d_o = -sigmoid(x) if d_h - d_o <= c, else 0;
 *   case B  O and both and d_h < d_o: x = min(d_o - d_h, c), the same with the sign +.   Equal depths contribute nothing.
 * Orientation: face_index is chore_silhouette_fwd's (rows NOT flipped); occluder_depth, image_ref, keep_mask and coef are in
 * the orientation of SilLossROI.image_ref, i.e. their row r is row S - 1 - r of face_index.  S <= 4096, B <= 65535.
 * Every call runs on `stream`, allocates nothing, reads no device value on the host (it can be captured into a graph), uses
 * no float atomics and returns CHORE_EINVAL before any launch for NULL pointers and shapes it does not take.
 *
 * chore_sil_depth: depth[b, r, x] = d of the winner face_index[b, y, x], far_z where it is -1; r = S - 1 - y if flip_rows,
 *   else y.  With flip_rows it equals the depth image of chore_render_fwd at ssaa 1 bit for bit.  Fills occluder_depth.
 * chore_ordinal_depth_fwd: per_frame_sum (B) = the sum of the terms over the frame's pixels; coef (B,S,S) = d term / d d_o, 0
 *   wherever neither case holds; counts (B,4) int32 = pixels in case A, in case B, in P and both, in O and both.  The sum is a
 *   tree over blocks of 256 pixels (8 additions deep), then per frame thread t adds block sums t, t + 256, ... and the same
 *   tree follows: the longest chain is 16 + ceil(ceil(S^2 / 256) / 256) additions.  expf / log1pf are the device library's.
 *   0 < c <= 80.  workspace: chore_ordinal_depth_workspace_bytes(B, S) (0 = unsupported shape).
 * chore_ordinal_depth_bwd: grad_tri (B,F,3,3), overwritten = the depth rule of chore_render_bwd, all three components, applied
 *   to the per-pixel depth gradient coef[b, r, x] * g_per_frame[b] (one float product): bit for bit what chore_render_bwd gives
 *   for that product as grad_depth alone.  Gathered per face: a workgroup walks the face's box, every thread adds the pixels
 *   the face won in tile order, then a fixed butterfly per wave and the four waves in order.  Faces that won nothing get zeros.
 * ------------------------------------------------------------------------------------------- */
int chore_sil_depth(chore_handle* h, const float* tri, const int* face_index, int B, int F, int S, float far_z, int flip_rows,
                    float* depth, chore_stream_t stream);
size_t chore_ordinal_depth_workspace_bytes(int B, int S);
int chore_ordinal_depth_fwd(chore_handle* h, const float* tri, const int* face_index, const float* occluder_depth,
                            const float* image_ref, const float* keep_mask, int B, int F, int S, float far_z, float c,
                            float* per_frame_sum, float* coef, int* counts, void* workspace, chore_stream_t stream);
int chore_ordinal_depth_bwd(chore_handle* h, const float* tri, const int* face_index, const float* coef, const float* g_per_frame,
                            int B, int F, int S, float* grad_tri, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Colour / depth / coverage rendering of meshes  (replaces what Renderer.render gets from neural_renderer's
 * rasterize_rgbad, external/neural_renderer/neural_renderer/rasterize.py:267-348: forward_face_index_map,
 * forward_texture_sampling, forward_background and forward_alpha_map of cuda/rasterize_cuda_kernel.cu:24-288 at image
 * size `size * ssaa`, the vertical flip and the 2x2 average of anti_aliasing=True).
 * tri (B,F,3,3) projected triangles [u, v in [-1,1], depth] with both windings already in the list; textures
 * (B,F,ts,ts,ts,3), ts >= 2; light (B,F,3) per-face factor or NULL = 1 (the reference multiplies the textures by it
 * beforehand, lighting.py:55-56; here the blended texel is multiplied); background3: HOST, 3 floats; ssaa 1 or 2.
 * Per sample: the hit rule of chore_silhouette_fwd at size * ssaa (the winning face is bit-identical to it: smallest
 * depth, then smallest face index; no face is dropped; a sample is tested against exactly the triangles whose box meets
 * its aligned 16 x 16-sample tile, as there, so zero-area triangles resolve alike too), colour = trilinear blend of the face's texture cube at
 * clamp(w_k (ts-1) zp / z_k, 0, ts-1-tex_eps) times light, background3 where nothing was hit; depth zp or far_z; alpha 1 or 0.
 * Outputs are resolved: row r holds sample rows of block size-1-r (the reference's flip), the mean over the ssaa x ssaa
 * samples for rgb (B,3,size,size), depth (B,size,size) and alpha (B,size,size) alike.  sample_face_index
 * (B,size*ssaa,size*ssaa) int32 or NULL: the winner of every sample, -1 = none, rows NOT flipped (like
 * chore_silhouette_fwd).  size * ssaa <= 4096.  chore_render_workspace_bytes depends on the shapes only (0 = unsupported
 * shape); nothing is allocated and no device value is read by the host, so the call can be captured into a graph.
 * ------------------------------------------------------------------------------------------- */
size_t chore_render_workspace_bytes(int B, int F, int size, int ssaa);
int chore_render_fwd(chore_handle* h, const float* tri, const float* textures, const float* light, int B, int F, int ts,
                     int size, int ssaa, float near_z, float far_z, float tex_eps, const float* background3, float* rgb,
                     float* depth, float* alpha, int* sample_face_index, void* workspace, chore_stream_t stream);
/* The backward of chore_render_fwd (replaces backward_pixel_map with rgb, backward_textures and backward_depth_map,
 * cuda/rasterize_cuda_kernel.cu:290-638, as RasterizeFunction.backward calls them, rasterize.py:114-170).  tri, textures,
 * light, the sizes, tex_eps and background3 (HOST) are the forward's arguments, sample_face_index its output.  grad_rgb
 * (B,3,size,size), grad_depth, grad_alpha (B,size,size): the upstream gradients, each may be NULL, and NULL gives the bits an
 * all-zero gradient gives.  Outputs: grad_tri (B,F,3,3); grad_textures (B,F,ts,ts,ts,3) or NULL; grad_light (B,F,3) or NULL.
 * Rules, on the sample grid S = size * ssaa:
 *   - the upstream gradient of output pixel (r, x), divided by ssaa^2, goes to each of its samples in sample row block
 *     size-1-r (the forward's flip and average), for rgb, depth and alpha alike;
 *   - pixel map -> grad_tri[..., :2]: the edge walk of chore_silhouette_bwd with diff_grad = the alpha contribution plus the
 *     three rgb contributions, summed before the diff_grad <= 0 gate; sample colours are the forward's (texel x light, or
 *     background3), `eps` is added to the distance; back faces get nothing.  Not run when grad_rgb and grad_alpha are both
 *     NULL (the reference's return_rgb = return_alpha = False of render_depth).  With grad_alpha alone at ssaa 1 the result
 *     is chore_silhouette_bwd's bit for bit (its rows are not flipped: hand grad_alpha over with the rows reversed);
 *   - depth -> grad_tri, all three components, from every sample a face won: with w the sample's weights and d its depth,
 *     d z_k += g w_k d^2 / z_k^2 and d (x, y)_k += g w_k d^2 (S / 2) sum_l inv[3 l + (x, y)] / z_l, inv the pixel-space inverse;
 *   - textures: the eight trilinear taps of the forward's sampling rule (clamp ts-1-tex_eps) weighted by the sample's rgb
 *     gradient times light; light: the sample's rgb gradient times the blended texel, summed over the face's samples.
 * Nothing is added atomically: the pixel-map term has one writer per face, the other terms are gathered per face (a
 * workgroup walks the face's box and sums the samples it won in a fixed order), so results are bit-equal from call to call
 * and under graph replay.  workspace: chore_render_bwd_workspace_bytes(B, F, ts, size, ssaa) bytes, 256-byte aligned, from
 * the shapes alone (0 = unsupported shape: ssaa not 1 or 2, ts < 2, size * ssaa > 4096); it holds 36 bytes per sample.
 * Everything runs on `stream`, nothing is allocated and no device value is read by the host, so forward + backward can be
 * captured into one graph.  near_z / far_z are the forward's (a winner has passed them; not read). */
size_t chore_render_bwd_workspace_bytes(int B, int F, int ts, int size, int ssaa);
int chore_render_bwd(chore_handle* h, const float* tri, const float* textures, const float* light,
                     const int* sample_face_index, int B, int F, int ts, int size, int ssaa, float near_z, float far_z,
                     float tex_eps, float eps, const float* background3, const float* grad_rgb, const float* grad_depth,
                     const float* grad_alpha, float* grad_tri, float* grad_textures, float* grad_light, void* workspace,
                     chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Point clouds as shaded discs, forward only  (what the reference's -d viewer shows, recon/recon_fit_base.py:442-511,
 * 749-845, is all point clouds; there is no counterpart kernel in the reference, the rule below is this library's own).
 * pts (B,N,3) projected points [u, v in [-1,1], depth], the layout of chore_render_fwd's triangle vertices; rgb_in (B,N,3)
 * or NULL = white; radius (B,N) in OUTPUT pixels or NULL = radius_px for every point; ambient in [0,1]; background3: HOST,
 * 3 floats; ssaa 1 or 2; size * ssaa <= 4096; B, N >= 1.  Sample grid S = size * ssaa, all arithmetic fp32, each operation
 * rounded once (no contraction), in the association written here:
 *   - point n is skipped if u, v, z or r is NaN, if r <= 0, or if z <= near_z || far_z <= z (chore_render_fwd's depth test);
 *   - rs = fminf(r * ssaa, 64): larger radii are clamped, not refused;
 *   - px = 0.5f * ((u * S + S) - 1.0f), py alike from v: where chore_render_fwd puts a vertex at the same [u, v];
 *   - sample (column i, row j) is covered iff dx*dx + dy*dy <= rs*rs with dx = (float)i - px, dy = (float)j - py;
 *   - the winner of a sample is the covering point with the smallest z, then the smallest n, whatever the order of the
 *     points (a 64-bit integer atomicMin per sample: no float atomics, bit-equal across calls, permutations and replays);
 *   - colour = rgb_in[n] * (ambient + (1 - ambient) * sqrtf(fmaxf(0, 1 - d2 / (rs*rs)))), depth = z, alpha = 1; an empty
 *     sample is background3 / far_z / 0.
 * Outputs are resolved as chore_render_fwd's: row r holds the sample rows of block size-1-r, the mean over the
 * ssaa x ssaa samples for rgb (B,3,size,size), depth (B,size,size) and alpha (B,size,size) alike.  sample_point_index
 * (B,size*ssaa,size*ssaa) int32 or NULL: the winner of every sample, -1 = none, rows NOT flipped.
 * workspace: chore_splat_workspace_bytes(B, N, size, ssaa) bytes, 16-byte aligned (0 = unsupported shape); it depends on the
 * shapes only, nothing is allocated and no device value is read by the host, so the call can be captured into a graph.
 * CHORE_EINVAL, before anything is launched: a NULL pts / background3 / output / workspace, N < 1, B < 1, ssaa not 1 or 2,
 * size * ssaa > 4096, ambient outside [0,1], near_z >= far_z, radius == NULL with radius_px <= 0.
 * ------------------------------------------------------------------------------------------- */
size_t chore_splat_workspace_bytes(int B, int N, int size, int ssaa);
int chore_splat_fwd(chore_handle* h, const float* pts, const float* rgb_in, const float* radius, float radius_px, int B, int N,
                    int size, int ssaa, float ambient, float near_z, float far_z, const float* background3, float* rgb,
                    float* depth, float* alpha, int* sample_point_index, void* workspace, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Meshes and point clouds in one image, forward only  (what the reference's -d viewer shows in one view,
 * recon/recon_fit_base.py:442-511, 749-795: point clouds next to sphere and ground-truth MESHES; the rule is this library's own).
 * The triangle arguments (tri, textures, light, B, F, ts, tex_eps) are chore_render_fwd's, the point arguments (pts,
 * point_rgb, radius, radius_px, N, ambient) chore_splat_fwd's; size, ssaa, near_z, far_z, background3 (HOST) serve both.
 * face_opacity (B,F) or NULL = 1; point_depth_bias: a host scalar >= 0 in depth units.  F, N >= 1.
 * Per sample of the size * ssaa grid, all arithmetic fp32, each operation rounded once, in the association written here:
 *   - the face layer is exactly chore_render_fwd's: the winning face f (smallest zp, then smallest index, under the hit rule
 *     of chore_silhouette_fwd), its colour m = texture blend times light, its depth zf = zp;
 *   - the point layer is exactly chore_splat_fwd's: the winning point n (smallest z, then smallest index, by the 64-bit
 *     integer atomicMin key), its shaded colour p, its depth zn;
 *   - the point is in front iff a point covers the sample and (no face covers it, or zn - point_depth_bias < zf); equality
 *     goes to the face.  The bias exists because fitted clouds lie ON the fitted surface: without it about half of their
 *     points lose to their own mesh;
 *   - o = fminf(fmaxf(face_opacity[b,f], 0), 1), NaN -> 0: clamped on the device, the host reads no device value;
 *   - point in front: colour p, depth zn, alpha 1, sample_id = -2 - n;
 *   - face in front: under = p where a point covers the sample (necessarily behind), otherwise background3; colour = m
 *     untouched when o >= 1, otherwise o * m + (1 - o) * under (two products, one sum); depth zf; alpha 1 where a point
 *     covers the sample, otherwise o; sample_id = f;
 *   - nothing covers the sample: background3 / far_z / 0, sample_id = -1.
 * Two layers are the default, not the limit: here a translucent face shows the nearest point behind it or the background;
 * chore_scene_layers_fwd (below) lets it show further faces as well.
 * Outputs are resolved as chore_render_fwd's and chore_splat_fwd's: per output pixel the samples are summed in the order
 * s = sy * ssaa + sx starting from 0 and multiplied by 1 / ssaa^2, for rgb (B,3,size,size), depth (B,size,size) and alpha
 * (B,size,size) alike; row r holds the sample rows of block size-1-r.  sample_id (B,size*ssaa,size*ssaa) int32 or NULL, rows
 * NOT flipped.  With no point in view the outputs equal chore_render_fwd's bit for bit, with no face chore_splat_fwd's.
 * workspace: chore_scene_workspace_bytes(B, F, N, size, ssaa) bytes, 256-byte aligned: the render workspace, padded to 256
 * bytes, then the keys (0 = a shape either of the two refuses).  It depends on the shapes only; every launch goes on
 * `stream`, nothing is allocated and no device value is read by the host, so the call can be captured into a graph.
 * CHORE_EINVAL, before anything is launched: whatever chore_render_fwd or chore_splat_fwd refuses, F < 1, N < 1,
 * point_depth_bias negative or NaN.
 * ------------------------------------------------------------------------------------------- */
size_t chore_scene_workspace_bytes(int B, int F, int N, int size, int ssaa);
int chore_scene_fwd(chore_handle* h,
    const float* tri, const float* textures, const float* light, const float* face_opacity, int B, int F, int ts,
    const float* pts, const float* point_rgb, const float* radius, float radius_px, int N, float point_depth_bias,
    int size, int ssaa, float ambient, float near_z, float far_z, float tex_eps, const float* background3,
    float* rgb, float* depth, float* alpha, int* sample_id, void* workspace, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * chore_scene_fwd with several face layers: per sample a list of up to K = face_layers faces (1 <= K <= 8) is composited
 * front to back with the point layer and the background, so that a translucent mesh shows the meshes behind it.  The arguments
 * are chore_scene_fwd's plus face_group (B,F) int32 or NULL and face_layers.  g(f) = face_group[b,f] (any int32) when
 * face_group is given, otherwise g(f) = f: of the faces of one group only the nearest counts, so a translucent closed mesh
 * that is one group adds one layer and not also its own back side.
 * Per sample of the size * ssaa grid, all arithmetic fp32, each operation rounded once, in the association written here:
 *   1. candidates: every face that hits the sample under chore_render_fwd's hit rule (the aligned 16 x 16 tile box test of
 *      chore_silhouette_fwd included), with its depth zp.  A NaN zp is no candidate (it never wins in chore_render_fwd);
 *   2. grouping: of the candidates with equal g, the one with the smallest zp, then the smallest f, is kept;
 *   3. ordering: the survivors are ordered by (zp, f) ascending and the first K kept: e_1 .. e_m with depths z_i, faces f_i,
 *      colours m_i (texture blend times light, as chore_render_fwd) and opacities o_i = fminf(fmaxf(face_opacity[b,f_i], 0), 1),
 *      NaN -> 0, NULL = 1;
 *   4. the point layer is exactly chore_splat_fwd's: the winner n, its shaded colour p, its depth zn;
 *   5. e_i lies before the point iff not (a point covers the sample and zn - point_depth_bias < z_i); equality goes to the
 *      face.  Depths ascend, so these are a prefix e_1 .. e_j;
 *   6. the cut: v = the first i <= j with o_i >= 1, or j if there is none;
 *   7. v = 0: the point gives p / zn / 1 / sample_id -2 - n; without a point background3 / far_z / 0 / -1;
 *   8. v >= 1: under = p where a point covers the sample, otherwise background3.  Colour: c = under, then for i = v down to 1:
 *      c = m_i if o_i >= 1, else o_i * m_i + (1 - o_i) * c (two products, one sum).  depth = z_1, sample_id = f_1.
 *      alpha = 1 where a point covers the sample or o_v >= 1; otherwise a = 0, then for i = v down to 1: a = o_i + (1 - o_i) * a;
 *   9. resolve, flip and sample_id layout as chore_scene_fwd's.
 * Consequences: K = 1 is chore_scene_fwd's rule, with or without groups (the alpha fold gives o + (1 - o) * 0 = o), and runs
 * chore_scene_fwd's kernel.  Faces beyond the K nearest, faces behind the point and faces behind the first opaque face do not
 * exist for the sample.  A face of opacity 0 still takes a layer.  The result does not depend on the order in which the faces
 * are met (the kernel streams: a sorted list of K entries per sample in registers; a candidate of a listed group replaces
 * that entry if it is nearer by (zp, f) and is dropped otherwise, a candidate of a new group is inserted and entry K + 1 falls
 * off; the K-th depth never grows, so this keeps what steps 1-3 keep).
 * workspace: chore_scene_workspace_bytes, unchanged: the lists never reach memory.  The launches are chore_scene_fwd's, all
 * on `stream`; nothing is allocated or read back, so the call can be captured into a graph.
 * CHORE_EINVAL, before anything is launched: face_layers outside 1..8 and whatever chore_scene_fwd refuses.
 * ------------------------------------------------------------------------------------------- */
int chore_scene_layers_fwd(chore_handle* h,
    const float* tri, const float* textures, const float* light, const float* face_opacity, int B, int F, int ts,
    const float* pts, const float* point_rgb, const float* radius, float radius_px, int N, float point_depth_bias,
    int size, int ssaa, float ambient, float near_z, float far_z, float tex_eps, const float* background3,
    const int* face_group, int face_layers,
    float* rgb, float* depth, float* alpha, int* sample_id, void* workspace, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Instance masks and visibility of meshes, forward only  (replaces neural_renderer's mode='visibility':
 * external/neural_renderer/neural_renderer/renderer.py:79-117, visibility.py:12-34 and the atomicMax on face_visibility of
 * forward_face_index_map, cuda/rasterize_cuda_kernel.cu:200-205; and makes the masks BEHAVE ships per frame: the object as
 * seen, the object alone, the person).  Which mesh owns a sample, and which meshes would cover it if the others were not there.
 * tri (B,F,3,3) is chore_render_fwd's, both windings already in the list; face_group (B,F) int32 or NULL = every face in
 * group 0; 1 <= G <= 8; ssaa 1 or 2; size * ssaa <= 4096.  Per sample of the size * ssaa grid:
 *   1. candidates: every face that hits the sample under chore_render_fwd's hit rule (the aligned 16 x 16 tile box test of
 *      chore_silhouette_fwd and the near / far test included).  A NaN zp is no candidate (it never wins in chore_render_fwd);
 *   2. the winner f* is the candidate with the smallest zp, then the smallest index: bit-identical to chore_render_fwd's
 *      sample_face_index;
 *   3. g(f) = face_group[b,f].  A face whose group lies outside 0..G-1 is an occluder: it takes part in 1 and 2 and is
 *      counted in face_samples, and it belongs to no group.  The value is tested on the device, the host reads no device value;
 *   4. vis_g = 1 iff a winner exists and g(f*) == g;
 *   5. full_g = 1 iff at least one candidate has group g, whatever lies in front of it.
 * Outputs, each may be NULL: visible, full (B,G,size,size) fp32, resolved exactly as chore_render_fwd resolves alpha (the
 * samples summed in the order s = sy * ssaa + sx, times 1 / ssaa^2; row r holds sample row block size-1-r), so the values are
 * multiples of 1/4 or of 1 and exact; face_samples (B,F) int32: the number of samples face f wins; group_samples (B,G,2)
 * int32: the number of samples with vis_g, and with full_g; sample_face_index (B,size*ssaa,size*ssaa) int32, rows NOT
 * flipped, -1 = none.
 * The launches are a clear kernel (no memset node), chore_render_fwd's setup kernel and one tile kernel over the same bins, all
 * on `stream`.  The counts are integer sums
 * (group_samples: reduced in the workgroup to one integer add per workgroup, group and kind; face_samples: equal winners among
 * a lane's samples merged before the add); there are no float atomics, so every output is bit-equal from call to call and
 * under graph replay.  The counters are zeroed inside the call on `stream`.
 * workspace: chore_instances_workspace_bytes(B, F, G, size, ssaa) bytes, 256-byte aligned: the render workspace (0 = a shape
 * chore_render_fwd refuses, or G outside 1..8).  It depends on the shapes only, nothing is allocated and no device value is
 * read by the host, so the call can be captured into a graph.
 * CHORE_EINVAL, before anything is launched: whatever chore_render_fwd refuses for these sizes, G outside 1..8, a NULL tri
 * or workspace, all five outputs NULL.
 * ------------------------------------------------------------------------------------------- */
size_t chore_instances_workspace_bytes(int B, int F, int G, int size, int ssaa);
int chore_instances_fwd(chore_handle* h, const float* tri, const int* face_group, int B, int F, int G, int size, int ssaa,
                        float near_z, float far_z, float* visible, float* full, int* face_samples, int* group_samples,
                        int* sample_face_index, void* workspace, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Photo textures and point visibility, forward only: the texture cube of every face filled from a photo at the texels the
 * camera sees, and whether a projected point is seen.  (The rule is this library's own; neural_renderer has no counterpart.)
 * tri (B,F,3,3) projected triangles [u, v in [-1,1], depth], chore_render_fwd's; depth (B,S,S) depth of the nearest face per
 * sample of the ssaa-1 grid, rows NOT flipped, far_z where there is none: what chore_silhouette_fwd + chore_sil_depth(...,
 * flip_rows = 0) give, and chore_render_fwd at ssaa 1 with the rows reversed; photo (B,3,Hp,Wp) fp32 planar, Wp the side of the
 * square [-1,1]^2 maps to, of which the upper Hp <= Wp rows exist; fallback (B,F,3): the colour of a texel that gets none from the
 * photo; depth_bias in the depth units of the triangles; textures (B,F,ts,ts,ts,3): chore_render_fwd's layout; texel_visible
 * (B,F,ts,ts,ts) bytes 0 / 1, or NULL.  pts (B,N,3) projected points; visible (B,N) int32 0 / 1.
 * Texel (i,j,k) of face f of image b, vertices (u_k, v_k, z_k); all arithmetic fp32, each operation rounded once (no
 * contraction), sums of three from the left:
 *   1. weights: w = (i,j,k) / (i+j+k); the texel (0,0,0) takes (1/3,1/3,1/3).  The renderer samples the cube at
 *      w_k (ts-1) z / z_k, so the taps it blends sit at these normalised weights;
 *   2. depth: z = w0 z0 + w1 z1 + w2 z2; not visible unless near_z < z && z < far_z (NaN and degenerate vertices fall here);
 *   3. screen position: s_k = (w_k z_k) / z, u = sum s_k u_k, v = sum s_k v_k: the inverse of the renderer's texel rule;
 *   4. sample: px = 0.5f * ((u * S + S) - 1.0f), py alike from v, xi = floorf(px + 0.5f), yi = floorf(py + 0.5f); not visible
 *      outside 0..S-1;
 *   5. visible iff z <= depth[b, yi, xi] + depth_bias;
 *   6. photo position, only if visible: align_corners == 0: qx = 0.5f * ((u * Wp + Wp) - 1.0f), qy = 0.5f * (((-v) * Wp + Wp) - 1.0f);
 *      otherwise qx = ((u + 1) * 0.5f) * (Wp - 1), qy = ((1 - v) * 0.5f) * (Wp - 1) (grid_sample's align_corners=True).  In the
 *      photo iff -0.5 <= qx <= Wp - 0.5 && -0.5 <= qy <= Hp - 0.5.  Colour: x0 = floorf(qx), fx = qx - x0, rows alike; the taps
 *      x0, x0 + 1 clamped to 0..Wp-1 and y0, y0 + 1 to 0..Hp-1; top = a + (b - a) fx, bot = c + (d - c) fx, top + (bot - top) fy;
 *   7. textures = the photo colour if visible and in the photo, else fallback[b,f]; texel_visible = steps 2-5, whatever 6 says.
 * chore_point_visibility is steps 2, 4 and 5 on (u, v, z) = pts[b,n]: the same device function.
 * Both calls are one kernel on `stream`: no workspace, no allocation, no atomics, no device value read by the host (they can be
 * captured into a graph), bit-equal from call to call.  Index arithmetic is size_t.
 * CHORE_EINVAL, before anything is launched: a NULL required pointer, B, F, N < 1, ts outside 2..16, S outside 1..4096, Hp < 1,
 * Wp < 1, Hp > Wp.
 * ------------------------------------------------------------------------------------------- */
int chore_photo_textures_fwd(chore_handle* h, const float* tri, const float* depth, const float* photo,
                             const float* fallback, int B, int F, int ts, int S, int Hp, int Wp,
                             float near_z, float far_z, float depth_bias, int align_corners,
                             float* textures, unsigned char* texel_visible, chore_stream_t stream);
int chore_point_visibility(chore_handle* h, const float* pts, const float* depth, int B, int N, int S,
                           float near_z, float far_z, float depth_bias, int* visible, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Textured OBJ files, forward only: texture cubes from UV triangles and texture images (neural_renderer's load_textures) and one
 * image with a tile per face from texture cubes (neural_renderer's create_texture_image).  Both keep the reference's results
 * wherever the reference is defined, and say what happens where it is not.
 *
 * chore_load_textures.  uv (F,3,2) fp32; face_image (F) int32: index into the image table, or negative; face_color (F,3) fp32;
 * images: bytes on the device, all texture images back to back, each (H,W,3) RGB in file row order; images_bytes: their total;
 * image_off (M) byte offset of each image in `images` and image_hw (M,2) its H, W: HOST arrays, read and checked before the launch
 * and passed to the kernel by value; wrapping: 0 REPEAT, 1 MIRRORED_REPEAT, 2 CLAMP_TO_EDGE, 3 CLAMP_TO_BORDER; bilinear 0 / 1;
 * textures (F,ts,ts,ts,3) fp32, chore_render_fwd's layout, every element written.  One launch for all materials.
 * Texel (i,j,k) of face f; all arithmetic fp32, each operation rounded once (no contraction), sums of three from the left:
 *   1. face_image[f] < 0 (or >= M): the texel is face_color[f].  Done.
 *   2. wrapping == 3: the texel is 0.  (The reference writes zeros on every textured face in this mode and never samples; kept.)
 *   3. weights: d = (i,j,k) / (ts-1), s = d0 + d1 + d2, and d /= s if s > 0.  The texel (0,0,0) keeps three zero weights and so
 *      samples position (0,0): the reference's rule, not the 1/3 of chore_photo_textures_fwd.
 *   4. wrap the six coordinates, in registers (the reference rewrites `uv` from every texel thread of a face; `uv` is const here):
 *      mod(x,y) = x > 0 ? fmodf(x,y) : y + fmodf(x,y); REPEAT: mod(x,1), which sends 0 to 1 and 1 to 0 as in the reference;
 *      MIRRORED_REPEAT: mod(x,2) < 1 ? mod(x,1) : 1 - mod(x,1); CLAMP_TO_EDGE: min(max(x,0),1).  A face with a non-finite
 *      coordinate takes face_color[f] on every texel.
 *   5. position: pos_x = (u0 d0 + u1 d1 + u2 d2) (W-1), pos_y alike from v with (H-1), measured in the vertically flipped image:
 *      row r of the flipped image is row H-1-r of the image in `images` (flipped in the index; no copy is made).
 *   6. bilinear: x0 = (int)pos_x, fx = pos_x - x0, x1 = x0 + 1, rows alike; a pixel is (float)byte / 255.0f;
 *      top = a + (b - a) fx, bot = c + (d - c) fx, top + (bot - top) fy, so equal taps give their value exactly (the reference sums
 *      four weighted taps).  Nearest: roundf (half away from zero).  In both modes every index is clamped to 0..W-1 / 0..H-1
 *      before it is used (the reference's nearest mode and large bilinear positions are not): no load leaves the image.
 * CHORE_EINVAL, before anything is launched: a NULL uv, face_image, face_color or textures; F < 1; ts outside 2..16; M < 0 or
 * M > 128; with M > 0 a NULL images, image_off or image_hw, an H or W < 1, an image that does not lie inside images_bytes; a
 * wrapping outside 0..3.
 *
 * chore_texture_atlas.  textures (F,tsi,tsi,tsi,3) fp32; image (tile_h tso, tile_w tso, 3) fp32 in file row order (the first
 * row is the top of the picture), every element written.  Tile counts in integer arithmetic: tile_w = (int)sqrt(F-1) + 1,
 * tile_h = (F-1) / tile_w + 1 (the reference's Python divides truly under torch >= 1.5).  chore_texture_atlas_size gives
 * height = tile_h tso and width = tile_w tso, or CHORE_EINVAL where F < 1, tso < 2 or a side exceeds 16384 px.
 * Pixel (x, y), y counted from the bottom of the picture (it is written to row height-1-y); fp32 as above:
 *   1. col = x / tso, row = y / tso, fn = col + row tile_w, lx = x % tso, ly = y % tso, T = tso - 1.
 *   2. fn >= F: the pixel is 0.  (The reference indexes faces that do not exist here.)
 *   3. ly + 1 == lx: the steps below are evaluated at lx - 1.  (The reference's second kernel, which copies the left neighbour
 *      into these pixels; folded in, so no pixel reads another thread's output.)
 *   4. weights: w0 = ((T - ly) / T) / (1 + 1e-5f), w1 = ((ly - lx) / T) / (1 + 1e-5f), w2 = (lx / T) / (1 + 1e-5f): the
 *      reference's face_inv (x, y, 1) / (sum + eps) for its tile triangle p0 = tile corner, p1 = p0 + (0,T), p2 = p0 + (T,T),
 *      in tile-local coordinates (equal in exact arithmetic; accurate in fp32 at any atlas size, which the global form is not).
 *   5. t_q = min(max(w_q (tsi-1), 0), tsi-1 - 1e-5f), i_q = (int)t_q, f_q = t_q - i_q, upper index min(i_q + 1, tsi-1).  The
 *      pixel is the trilinear blend of the eight texels, in lerp form along k, then j, then i.
 *   6. pixels above the diagonal (lx > ly + 1) go through the same steps with w1 clamped to 0, as in the reference.
 * CHORE_EINVAL, before anything is launched: a NULL pointer, F < 1, tsi outside 2..16, tso < 2, a side above 16384 px.
 *
 * Both calls are one kernel on `stream`: no workspace, no allocation, no atomics, one writer per output element (bit-equal from
 * call to call), no device value read by the host.  Index arithmetic is size_t.
 * ------------------------------------------------------------------------------------------- */
int chore_load_textures(chore_handle* h, const float* uv, const int* face_image, const float* face_color,
                        const unsigned char* images, size_t images_bytes, const long long* image_off,
                        const int* image_hw, int M, int F, int ts, int wrapping, int bilinear, float* textures,
                        chore_stream_t stream);
int chore_texture_atlas_size(int F, int tso, int* height, int* width);
int chore_texture_atlas(chore_handle* h, const float* textures, int F, int tsi, int tso, float* image,
                        chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Evaluation metrics, fp64 (replace recon/eval/chamfer_distance.py:10-52 = sklearn kd-tree nearest neighbours, and
 * recon/eval/pose_utils.py compute_transform :145-180 / compute_similarity_transform :103-143).
 *   chore_eval_chamfer   out[0] = mean_i min_j |x_i - y_j| (direction 'x_to_y'), out[1] = the other direction
 *                        ('y_to_x'); 'bi' = out[0] + out[1].  Euclidean distances (not squared).  x (Nx,3), y (Ny,3) fp64.
 *   chore_eval_procrustes  params[13] = R (row-major), t, scale of the similarity that takes S1 closest to S2
 *                        (R = V Z U^T of K = X1 X2^T, det R = +1); chore_eval_apply_similarity: scale R p + t.
 * ------------------------------------------------------------------------------------------- */
size_t chore_eval_chamfer_workspace_bytes(int Nx, int Ny);
int chore_eval_chamfer(chore_handle* h, const double* x, int Nx, const double* y, int Ny, double* out, void* workspace,
                       chore_stream_t stream);
int chore_eval_procrustes(chore_handle* h, const double* S1, const double* S2, int N, double* params,
                          chore_stream_t stream);
int chore_eval_apply_similarity(chore_handle* h, const double* pts, int N, const double* params, double* out,
                                chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Device-resident bookkeeping of the surface-point generator  (replaces the boolean-mask indexing, Python lists and CPU
 * randint of Generator.gen_pc_batch / parse_preds, recon/generator.py:149-188, 190-217).
 *   chore_gen_compact   order[b][j] = index of the j-th set byte of mask[b][0..N), counts[b] = number of set bytes
 *                       (the order of x[mask]).
 *   chore_gen_append    dst[b][c][offsets[b] + j] = src[b][c][order[b][j]] for j < counts[b]; element strides given for
 *                       (b, c, n) of src and dst, so (B,N,3) and (B,C,N) tensors both fit; entries past `cap` dropped.
 *   chore_gen_advance   offsets[b] += counts[b]; *total += min_b counts[b]   (generator.py:156-158).
 *   chore_gen_resample  out (B,M,3): if counts[b] > 1, samples[b][order[b][floor(u * counts[b])]] + sigma * noise, else
 *                       init[b][floor(u * Ninit)] + 0.5 * noise (generator.py:163-177); u (B,M) uniform in [0,1), noise
 *                       (B,M,3) standard normal, both drawn by the caller on the device.
 * ------------------------------------------------------------------------------------------- */
int chore_gen_compact(chore_handle* h, const unsigned char* mask, int B, int N, int* order, int* counts,
                      chore_stream_t stream);
int chore_gen_append(chore_handle* h, const float* src, long long ss_b, long long ss_c, long long ss_n, const int* order,
                     const int* counts, const int* offsets, float* dst, long long ds_b, long long ds_c, long long ds_n,
                     int B, int C, int N, int cap, chore_stream_t stream);
int chore_gen_advance(chore_handle* h, const int* counts, int B, int* offsets, int* total, chore_stream_t stream);
int chore_gen_resample(chore_handle* h, const float* samples, int B, int N, const int* order, const int* counts,
                       const float* init, int Ninit, const float* u, const float* noise, int M, float sigma, float* out,
                       chore_stream_t stream);
/* one projection step of Alg. 1 (Generator.approx_surface, recon/generator.py:50-79) around chore_query_fwd /
 * chore_query_bwd_points: chore_gen_clamp_mask writes the upstream gradient of sum(clamp(df[:, k], max = thr)) -- g (B,2,N):
 * 1 where df[b,k,n] <= thr, else 0, the other channel 0 --, chore_gen_surface_step moves the points:
 * out = points - normalize(grad) * min(df[:, k], thr), normalize as F.normalize (v / max(||v||, 1e-12)) */
int chore_gen_clamp_mask(chore_handle* h, const float* df, int k, float thr, int B, int N, float* g, chore_stream_t stream);
int chore_gen_surface_step(chore_handle* h, const float* points, const float* grad, const float* df, int k, float thr, int B,
                           int N, float* out, chore_stream_t stream);
/* the four launches above (chore_query_fwd -> chore_gen_clamp_mask -> chore_query_bwd_points -> chore_gen_surface_step) as
 * one, with the same result bit for bit: arguments as chore_query_fwd; only with the fp16 x 3 heads (dtype CHORE_F16X3, or
 * the maps' type | CHORE_HEADS_X3).  out_points (B,N,3) must not alias points. */
int chore_gen_surface_step_fused(chore_handle* h, const float* points, const float* crop_center, int B, int N,
                                 const void* feat, int FH, int FW, const void* tmpx, int TH, int TW, int dtype,
                                 const void* heads_arena, const float* cam6_host, int k, float thr, float* out_points,
                                 chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Image preparation of the test loader on the device  (replaces, from the decoded uint8 images on,
 * TestData.prepare_image_crop data/test_data.py:59-125 with use_mean_center=False = BaseDataset.masks2bbox
 * data/base_data.py:92-112 + cv2.resize + BaseDataset.crop :131-162 + BaseDataset.resize :164-176 + compose_images
 * :178-192).  Integer arithmetic; cv2's 8-bit INTER_LINEAR algorithm is restated (oracle/image_prep.py): PARITY
 * UNPINNED at cv2, which the reference neither vendors nor pins.
 *   chore_prep_masks2bbox    bbox4 = {xmin, ymin, xmax + 1, ymax + 1} (int32, device) of the pixels where the uint8
 *                            wrap-around sum mask0 + mask1 exceeds thres; {50000, 50000, -100, -100} when there is none.
 *                            mask1 may be NULL.
 *   chore_prep_resize_u8     (sh, sw, C) uint8 -> (dh, dw, C) uint8, C <= 4.
 *   chore_prep_crop_compose  crop of the (H, W) images with corners tl = round(center - size / 2), br = round(center +
 *                            size / 2) (zero padded, base_data.py's clipping), resized to S x S, / 255, RGB zeroed where
 *                            neither mask exceeds 0.5, stacked as images (5, S, S) fp32 = [R, G, B, person, object].
 *                            rgb (H, W, 3), masks (H, W) uint8.
 * ------------------------------------------------------------------------------------------- */
int chore_prep_masks2bbox(chore_handle* h, const unsigned char* mask0, const unsigned char* mask1, int H, int W, int thres,
                          int* bbox4, chore_stream_t stream);
int chore_prep_resize_u8(chore_handle* h, const unsigned char* src, int sh, int sw, int C, unsigned char* dst, int dh, int dw,
                         chore_stream_t stream);
int chore_prep_crop_compose(chore_handle* h, const unsigned char* rgb, const unsigned char* person_mask,
                            const unsigned char* obj_mask, int H, int W, int tl_x, int tl_y, int br_x, int br_y, int S,
                            float* images, chore_stream_t stream);
/* use_mean_center=True (the COCO loader, recon/recon_fit_coco.py:28; data/test_data.py:127-160): the images are moved so
 * that the crop centre (cc, in the 2048-px space) lands on the mean crop centre of the BEHAVE training set (pad_image's
 * zero float64 canvas, at least 2048 x 1536, the pasted part clipped to that rectangle), the crop with corners tl / br is
 * taken around the mean centre, and the resize is cv2's generic float path (float weights, double sums) -- restated in
 * oracle/image_prep.py, UNPINNED like the 8-bit one. */
int chore_prep_crop_compose_mean(chore_handle* h, const unsigned char* rgb, const unsigned char* person_mask,
                                 const unsigned char* obj_mask, int H, int W, double cc_x, double cc_y, double mean_x, double mean_y,
                                 int tl_x, int tl_y, int br_x, int br_y, int S, float* images, chore_stream_t stream);

/* Image preparation of the TRAINING loader (BehaveDataset.prepare_image_crop data/train_data.py:134-149 on BaseDataset
 * data/base_data.py:71-192, from the decoded uint8 images on): the augmentations and the batched crop / compose.
 *   chore_prep_blur_u8       PIL.ImageFilter.GaussianBlur on src (B, H, W, C) uint8, C <= 4, -> dst (same shape; may be
 *                            src), bit for bit: three box-blur passes along the rows, then three along the columns, in
 *                            PIL's 24-bit fixed point, every pass rounded to uint8.  params (B, 3) int32 ON THE DEVICE holds
 *                            per image {R, ww, fw}: the integer part of the effective box radius, the weight of a whole
 *                            pixel and of the two fractional end pixels (TrainImagePrep.box_params computes them from the
 *                            PIL radius with PIL's float32 expressions); {0, 0, 0} copies the image.  max_r is the
 *                            largest R in params, declared by the caller, who filled them: above
 *                            chore_prep_blur_max_radius() (64, i.e. PIL radii up to about 64) the call is refused with
 *                            CHORE_EINVAL.  Whole lines are staged through LDS, so an R beyond the image's side is
 *                            covered; a line that does not fit the LDS (W * C above about 80 KB, H above about 20 000)
 *                            is refused.  workspace: chore_prep_blur_workspace_bytes(B, H, W, C) bytes, the one
 *                            intermediate image.  Two launches, no host read, no atomics, no allocation: records into a
 *                            hipGraph.
 *   chore_prep_train_compose chore_prep_crop_compose on a batch: rgb (B, H, W, 3), masks (B, H, W), HOST arrays
 *                            tlbr_host (B, 4) = {tl_x, tl_y, br_x, br_y} and flip_host (B), images (B, 5, S, S) fp32.
 *                            flip_host[b] != 0 takes the crop from the horizontal mirror of image b (column W - 1 - x of
 *                            all three sources); without it image b's result is chore_prep_crop_compose's bit for bit. */
int chore_prep_blur_max_radius(void);
size_t chore_prep_blur_workspace_bytes(int B, int H, int W, int C);
int chore_prep_blur_u8(chore_handle* h, const unsigned char* src, int B, int H, int W, int C, const int* params, int max_r,
                       unsigned char* dst, void* workspace, chore_stream_t stream);
int chore_prep_train_compose(chore_handle* h, const unsigned char* rgb, const unsigned char* person_mask,
                             const unsigned char* obj_mask, int B, int H, int W, const int* tlbr_host, const int* flip_host,
                             int S, float* images, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Interpenetration term of the joint fit  (replaces ReconFitterBase.smpl_obj_collision recon/recon_fit_base.py:610-624 =
 * mesh_intersection.BVH(max_collisions=8) + DistanceFieldPenetrationLoss(sigma=0.5, point2plane=False), constructed at
 * :78-86).  PARITY UNPINNED: that package (github.com/vchoutas/torch-mesh-isect, no revision pinned) is not in the
 * reference tree; oracle/collision.py states the published method implemented here.
 *   verts  (B,V,3) fp32: the concatenated mesh (SMPL vertices, then object vertices), faces (F,3) int32 into it.
 *   loss   (B) per-batch-element sums over all intersecting, non-adjacent triangle pairs (the caller takes the mean,
 *          like torch.mean(self.pen_distance(...)) :623);  gverts (B,V,3) = d loss[b] / d verts[b], kept for backward;
 *          A triangle whose normal is exactly zero in fp32 has no cone and no interior: it takes part in no pair.
 *   counts (B+2 int32, or NULL): pairs kept per batch element, then candidates / pairs dropped for lack of list space
 *          (24 F + 4096 candidates, 8 F + 1024 pairs per element; which ones survive a full list is not defined).
 * chore_collision_bwd: dverts = gout[b] * gverts.  No host synchronisation, fixed launch grids (hipGraph-capturable),
 * fixed-point accumulation (bit-reproducible).
 * ------------------------------------------------------------------------------------------- */
size_t chore_collision_workspace_bytes(int B, int V, int F);
int chore_collision_fwd(chore_handle* h, const float* verts, const int* faces, int B, int V, int F, float* loss,
                        float* gverts, int* counts, void* workspace, chore_stream_t stream);
int chore_collision_bwd(chore_handle* h, const float* gverts, const float* gout, int B, int V, float* dverts,
                        chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Encoder layers as differentiable operators (training path).  Replace what torch autograd runs for
 * the reference's encoder modules: nn.Conv2d 3x3 / 1x1 (model/net_util.py:346-349, 356-372,
 * model/HGFilters.py:88-116), nn.GroupNorm(32, C) + F.relu (model/net_util.py:374-396, HGFilters.py:153-176),
 * F.interpolate(scale 2, bicubic, align_corners=True) + add (HGFilters.py:47-50), and their backward passes.
 * The host (chore_amd/ops.py, model/hgfilter_train.py) wires them into torch.autograd.Function nodes.
 *
 * Activations: NHWC (B,H,W,C), `dtype` = CHORE_F32, CHORE_BF16 or -- round 5 -- CHORE_F16X3 (fp32 tensors; every convolution,
 * data gradient and weight gradient on the fp16 matrix cores with hi / lo split operands, fp32-grade: the mode that trains at the
 * reference's precision, trainer/trainer.py:76-85, at matrix-core speed).  Parameters and parameter gradients: fp32
 * in the reference layouts (weight (Cout,Cin,k,k), bias/gamma/beta (C)).  taps = 1 (1x1) or 9 (3x3, pad 1).
 * C, Cin, Cout multiples of 32.  `stats`: chore_gn_stats_bytes(B) bytes, the exact per-(image, group)
 * sum / sum of squares of x, filled by chore_gn_stats; wherever an operator takes (stats, gamma, beta) != NULL
 * it sees relu(groupnorm(x)) instead of x, applied while the tile is staged (the normalised tensor is never
 * written).  Workspaces are caller-owned, sized by the *_bytes functions, and may be reused between calls on
 * one stream.  All reductions are order-fixed (integer accumulators or ordered partial sums): results are
 * bit-reproducible run to run.
 * ------------------------------------------------------------------------------------------- */
size_t chore_conv2d_workspace_bytes(int dtype, int taps, int Cin, int Cout);
size_t chore_gn_stats_bytes(int B);
/* CHORE_F16X3 training: a gradient that feeds a data- or weight-gradient GEMM has any magnitude, while an fp16 hi / lo pair keeps
 * 22 bits only for |x| in 2^-3 .. 2^16; the kernels therefore scale it by a power of two derived from max |x|, which travels
 * with the tensor: chore_amax_bytes() bytes of partial maxima (float bits), written by chore_absmax_f32 (n a multiple of 4,
 * x 16-byte aligned) -- inside chore_convblock_bwd by the kernels that produce the gradients. */
size_t chore_amax_bytes(void);
int chore_absmax_f32(chore_handle* h, const float* x, size_t n, void* amax, chore_stream_t stream);
/* zeroed != 0: `stats` already holds zeros (a slice of an arena cleared once per pass) */
int chore_gn_stats(chore_handle* h, int dtype, const void* x, int B, int HW, int C, void* stats, int zeroed,
                   chore_stream_t stream);
/* y = relu(groupnorm(x)) */
int chore_gn_relu_fwd(chore_handle* h, int dtype, const void* x, const void* stats, const float* gamma,
                      const float* beta, void* y, int B, int HW, int C, chore_stream_t stream);
/* y (B,H,W,Cout) = conv(a) + bias (bias may be NULL); out_stats (or NULL): ZEROED statistics accumulators filled with
 * the statistics of y by the convolution's epilogue (for a GroupNorm(32, Cout) that follows) */
int chore_conv2d_fwd(chore_handle* h, int dtype, int taps, const void* x, int B, int H, int W, int Cin,
                     const void* stats, const float* gamma, const float* beta, const float* w, const float* bias,
                     int Cout, void* y, void* out_stats, void* workspace, chore_stream_t stream);
/* chore_conv2d_fwd with a residual and a pooled output: y = conv(a) + bias + res (res (B,H,W,Cout) or NULL), y_pool (B,H/2,W/2,Cout) =
 * the 2x2 average of y exactly as chore_avgpool2_fwd forms it, pool_stats (or NULL): ZEROED accumulators for the statistics of
 * y_pool.  H and W even.  Where the convolution's epilogue can carry the pooled output (CHORE_F16X3, 3x3, GroupNorm fused) y may be
 * NULL: only y_pool is written.  Elsewhere the pooling runs as a pass over y (y required; Cout 64, 128 or 256) */
int chore_conv2d_pool_fwd(chore_handle* h, int dtype, int taps, const void* x, int B, int H, int W, int Cin,
                          const void* stats, const float* gamma, const float* beta, const float* w, const float* bias,
                          int Cout, const void* res, void* y, void* out_stats, void* y_pool, void* pool_stats, void* workspace,
                          chore_stream_t stream);
/* dx (B,H,W,Cin) = gradient w.r.t. the tensor the convolution saw (a).  dy_amax: chore_absmax_f32 of dy, required with
 * CHORE_F16X3 (NULL otherwise); the same for chore_conv2d_bwd_weight */
int chore_conv2d_bwd_data(chore_handle* h, int dtype, int taps, const void* dy, int B, int H, int W, int Cout,
                          const float* w, int Cin, void* dx, void* workspace, const void* dy_amax, chore_stream_t stream);
/* dw (Cout,Cin,k,k), dbias (Cout, or NULL) */
size_t chore_conv2d_wgrad_workspace_bytes(int taps, int B, int H, int W, int Cin, int Cout);
int chore_conv2d_bwd_weight(chore_handle* h, int dtype, int taps, const void* x, int B, int H, int W, int Cin,
                            const void* stats, const float* gamma, const float* beta, const void* dy, int Cout,
                            float* dw, float* dbias, void* workspace, const void* dy_amax, chore_stream_t stream);
/* da = gradient w.r.t. relu(groupnorm(x))  ->  dx, dgamma (C), dbeta (C) */
size_t chore_gn_relu_bwd_workspace_bytes(int B, int C);
int chore_gn_relu_bwd(chore_handle* h, int dtype, const void* x, const void* stats, const float* gamma,
                      const float* beta, const void* da, int B, int HW, int C, void* dx, float* dgamma,
                      float* dbeta, void* workspace, int workspace_zeroed, chore_stream_t stream);
/* One ConvBlock (reference model/net_util.py:346-396: three GroupNorm -> ReLU -> conv3x3 stages, their concat, and the
 * identity or GroupNorm -> ReLU -> conv1x1 residual) as a training operator, forward and backward in one call each: the
 * convolutions write their slices of y with the residual added in the epilogue and produce the GroupNorm statistics of
 * o1, o2 and y there; the backward reads dy in channel-strided slices and sums the skip gradients inside the GroupNorm
 * backward.  dtype: CHORE_F32 | CHORE_BF16 | CHORE_F16X3; Cout in {128, 256}, Cin a multiple of 32 (<= 256); conv weights in the
 * reference layout (O,C,kh,kw) fp32, no biases; wd and gb[6], gb[7] only when Cin != Cout.
 *   gb      host array of 8 device pointers: gamma, beta of bn1, bn2, bn3, bn4
 *   x_stats chore_gn_stats_bytes(B) statistics of x (the previous block's: `saved` + chore_convblock_out_stats_offset(B)),
 *           or NULL: computed by the forward (and kept in `saved` for the backward)
 *   saved   chore_convblock_saved_bytes: o1, o2 and all statistics, forward -> backward
 *   grads   chore_convblock_grad_floats: dW1 dW2 dW3 [dWd] then (dgamma, dbeta) of bn1, bn2, bn3 [, bn4] */
size_t chore_convblock_saved_bytes(int dtype, int B, int H, int W, int Cin, int Cout);
size_t chore_convblock_out_stats_offset(int B);
size_t chore_convblock_workspace_bytes(int dtype, int B, int H, int W, int Cin, int Cout);
size_t chore_convblock_grad_floats(int Cin, int Cout);
int chore_convblock_fwd(chore_handle* h, int dtype, const void* x, const void* x_stats, int B, int H, int W, int Cin,
                        int Cout, const float* w1, const float* w2, const float* w3, const float* wd,
                        const float* const* gb, void* y, void* saved, void* workspace, chore_stream_t stream);
int chore_convblock_bwd(chore_handle* h, int dtype, const void* x, const void* x_stats, const void* dy, int B, int H,
                        int W, int Cin, int Cout, const float* w1, const float* w2, const float* w3, const float* wd,
                        const float* const* gb, const void* saved, void* dx, float* grads, void* workspace,
                        chore_stream_t stream);
/* The training loss of one stack (reference model/chore.py:192-237, CHORE.get_errors) and its gradients with respect to
 * the four predictions, one pass: clamped-L1 of the two distance fields, cross entropy of the part logits, masked MSE of
 * the PCA axes and the two centre predictions.  losses: 7 device floats -- the six terms in the reference's order (h, o,
 * parts, pca, smpl, obj) and their sum, each times `scale`; accumulate != 0 adds to them.  weights: host array, the
 * reference's self.loss_weights.  g_*: gradients of the added sum.  Exact (order-independent) reductions. */
size_t chore_train_loss_workspace_bytes(void);
int chore_train_loss(chore_handle* h, const float* df, const float* pca, const float* parts, const float* centers,
                     const float* df_h, const float* df_o, const int64_t* parts_gt, const float* pca_gt,
                     const float* body_center, const float* obj_center, int B, int N, float max_dist,
                     const float* weights, float scale, float* g_df, float* g_pca, float* g_parts, float* g_centers,
                     float* losses, int accumulate, void* workspace, chore_stream_t stream);
/* y (B,2H,2W,C) = a + bicubic_up2(low (B,H,W,C));  d_low = transpose of the upsampling applied to dy */
/* out_stats (both operators; or NULL): ZEROED chore_gn_stats_bytes(B) accumulators that receive the GroupNorm statistics
 * of y from the same pass (what a ConvBlock consuming y takes as x_stats) */
int chore_upadd_fwd(chore_handle* h, int dtype, const void* a, const void* low, void* y, int B, int H, int W, int C,
                    void* out_stats, chore_stream_t stream);
int chore_up2_bwd(chore_handle* h, int dtype, const void* dy, void* dlow, int B, int H, int W, int C,
                  chore_stream_t stream);
/* y (B,H/2,W/2,C) = 2x2 average pooling of x (B,H,W,C) (nn.AvgPool2d / F.avg_pool2d(2, stride 2), HGFilters.py:33,153),
 * C in {64,128,256}; dx (B,H,W,C) = its transpose applied to dy */
int chore_avgpool2_fwd(chore_handle* h, int dtype, const void* x, void* y, int B, int H, int W, int C, void* out_stats,
                       chore_stream_t stream);
int chore_avgpool2_bwd(chore_handle* h, int dtype, const void* dy, void* dx, int B, int H, int W, int C,
                       chore_stream_t stream);
/* stem: y (B,H/2,W/2,64) = conv 7x7 stride 2 pad 3 of images (B,Cin,H,W) fp32 NCHW, + bias (model/HGFilters.py:102,149;
 * Cin <= 8 forward, <= 5 for the weight gradient; the images take no gradient).  dy has y's layout and dtype. */
size_t chore_stem_workspace_bytes(int Cin);
int chore_stem_fwd(chore_handle* h, int dtype, const float* images, int B, int Cin, int H, int W, const float* w,
                   const float* bias, void* y, void* workspace, chore_stream_t stream);
/* the stem of the CHORE_F16X3 mode (matrix cores, hi / lo split operands; Cin 3, 4 or 5): fp32 y (B,H/2,W/2,64) and, with out_stats
 * != NULL (ZEROED accumulators), the GroupNorm statistics of y from the same launch */
size_t chore_stem_x3_workspace_bytes(int Cin);
int chore_stem_x3_fwd(chore_handle* h, const float* images, int B, int Cin, int H, int W, const float* w, const float* bias,
                      void* y, void* out_stats, void* workspace, chore_stream_t stream);
size_t chore_stem_wgrad_workspace_bytes(int B, int Cin, int H, int W);
int chore_stem_bwd_weight(chore_handle* h, int dtype, const float* images, int B, int Cin, int H, int W, const void* dy,
                          float* dw, float* dbias, void* workspace, chore_stream_t stream);
/* C (M,N) = A^T B, fp32 (exact fp32 matrix-core arithmetic), A (P,M) row stride lda, B (P,N) row stride ldb;
 * M, N multiples of 32, any P.  The weight gradients of the MLP heads (what autograd computes for the
 * nn.Conv1d layers of model/net_util.py:218-262). */
size_t chore_gemm_tn_workspace_bytes(int P, int M, int N);
int chore_gemm_tn_f32(chore_handle* h, const float* A, int lda, const float* B, int ldb, int P, int M, int N,
                      float* C, void* workspace, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement aid (bench.py roofline): while enabled, chore_encode_fwd brackets every kernel launch
 * with hipEvents on the caller's stream, synchronises at the end of the call and accumulates, per
 * kernel class, the elapsed milliseconds, the algorithmic FLOPs and bytes and the launch count.
 * Enabling/disabling resets the counters.  Not for the timed region (it serialises the host).
 * chore_profile_read fills HOST arrays and returns the number of classes written.
 * ------------------------------------------------------------------------------------------- */
int chore_profile_enable(chore_handle* h, int on);
int chore_profile_read(chore_handle* h, int max_classes, const char** names, double* ms, double* flops,
                       double* bytes, int64_t* launches);

/* The tail of one inner fitting step (reference recon/recon_fit_behave.py:143-160, 270-287): Adam -- the formulas of
 * torch.optim.Adam(capturable=True) -- on nt <= 16 small fp32 tensors in one launch, and the early-stop rule
 * |prev - loss| / prev < prev * tol with its latch in another.  p / g / m / v: host arrays of device pointers, n: lengths;
 * step, prev, loss, loss_out: device floats; stop, armed: device bytes.  A set `stop` freezes the parameters (the moments and
 * the counter still advance).  chore_fit_stop_rule increments `step` (if not NULL): call it after chore_fit_adam_step. */
int chore_fit_adam_step(chore_handle* h, float* const* p, const float* const* g, float* const* m, float* const* v,
                        const int* n, int nt, const float* step, float lr, float beta1, float beta2, float eps,
                        const uint8_t* stop, chore_stream_t stream);
/* the same update with autograd's gradient accumulation folded in: g[k] is the ACCUMULATED gradient (the parameter's .grad,
 * read and written), gnew[k] (or NULL: nothing new) this step's fresh gradient, added to g[k] first -- the reference
 * accumulates over the inner steps of an outer iteration (recon_fit_behave.py:117-118,143-146), which as tensor ops is one
 * `grad += new` launch per parameter and step.  p[k] == NULL (then m[k], v[k] are ignored): a leaf that only accumulates
 * (stepped by a later phase's optimiser, which starts from these sums).  cols / pstride (host int arrays, or NULL = dense):
 * parameter k is a column slice of a wider tensor -- rows of cols[k] elements, pstride[k] apart (the split SMPL parameters of a
 * multi-frame batch, lib_smpl/wrapper_pytorch.py's SMPLPyTorchWrapperBatchSplitParams); g, gnew, m, v stay dense.  nt <= 16. */
int chore_fit_adam_step_acc(chore_handle* h, float* const* p, float* const* g, const float* const* gnew, float* const* m,
                            float* const* v, const int* n, const int* cols, const int* pstride, int nt, const float* step,
                            float lr, float beta1, float beta2, float eps, const uint8_t* stop, int step_counted,
                            chore_stream_t stream);   /* step_counted != 0: `step` already counts this step (see
                                                         chore_fit_weighted_sum_step) */
int chore_fit_stop_rule(chore_handle* h, const float* loss, float* prev, uint8_t* stop, const uint8_t* armed, float tol,
                        float* loss_out, float* step, chore_stream_t stream);
/* the weighting of the fit's loss dictionary (recon_fit_behave.py:339-358): out = sum_k coeff[k] * loss[k] / denom over
 * n <= 16 device scalars (losses: host array of device pointers; coeffs: host floats), and grads[k] = g * coeff[k] / denom */
int chore_fit_weighted_sum(chore_handle* h, const float* const* losses, const float* coeffs, int n, const float* denom,
                           float* out, chore_stream_t stream);
int chore_fit_weighted_sum_bwd(chore_handle* h, const float* coeffs, int n, const float* denom, const float* g, float* grads,
                               chore_stream_t stream);
/* The three single-thread launches of a step as one: chore_fit_weighted_sum, its backward for the upstream gradient *seed
 * (the step's d loss / d loss), and -- when prev != NULL -- chore_fit_stop_rule on the sum (recon_fit_behave.py:143-160,
 * 270-287).  The rule runs BEFORE the step's Adam launch here: `frozen` receives the stop flag as earlier steps left it
 * (hand THAT to chore_fit_adam_step_acc as `stop`: the reference applies the update of the step that meets the rule), and
 * `step` is advanced here (step_counted = 1 for the Adam launch). */
int chore_fit_weighted_sum_step(chore_handle* h, const float* const* losses, const float* coeffs, int n, const float* denom,
                                float* out, const float* seed, float* grads, float* prev, uint8_t* stop, uint8_t* frozen,
                                const uint8_t* armed, float tol, float* loss_out, float* step, chore_stream_t stream);

/* The small loss terms of forward_smpl (recon_fit_behave.py:293-337) in one launch each way.  pose (B,156) SMPL-H
 * axis-angle, pose_init (B,69) = the initial pose[3:72], J (B,R,3) landmarks whose first 25 rows are the body-25 keypoints
 * (row 8 = MidHip), kpts (B,25,3) = (x, y, confidence) in pixels of the network input or NULL (no keypoint term),
 * crop_center (B,2); body prior mean (63) / precision (63,63) applied to pose[3:66] (th_smpl_prior.py:32-39), hand prior
 * mean (90) and the two (45,45) precisions applied to pose[66:156] (th_hand_prior.py:63-72, incl. its sum over frames and
 * hands / 45); cam8 = HOST floats {fx, fy, cx, cy in pixels, crop/2, crop, network input size, z_0}.
 * out5 / up5: HOST arrays of 5 device scalars in the order pose prior, hand prior, pose-init, depth (smplz), keypoints (j2d);
 * a NULL entry of up5 is a zero gradient.  dpose (B,156) and dJ (B,R,3) are written completely. */
int chore_fit_smpl_terms_fwd(chore_handle* h, const float* pose, const float* pose_init, const float* J, const float* kpts,
                             const float* crop_center, const float* body_mean, const float* body_prec, const float* hand_mean,
                             const float* lhand_prec, const float* rhand_prec, int B, int P, int R, const float* cam8,
                             float* const* out5, chore_stream_t stream);
int chore_fit_smpl_terms_bwd(chore_handle* h, const float* pose, const float* pose_init, const float* J, const float* kpts,
                             const float* crop_center, const float* body_mean, const float* body_prec, const float* hand_mean,
                             const float* lhand_prec, const float* rhand_prec, int B, int P, int R, const float* cam8,
                             const float* const* up5, float* dpose, float* dJ, chore_stream_t stream);
/* Per-point terms: out_clamped_mean = mean over (B,N) of min(df[:, channel, :], clamp_max)  (df_h with channel 0 / 0.1,
 * recon_fit_base.py:520-526; the object term with channel 1 / 0.8, :505-511) and, if logits (B,C,N) is not NULL,
 * out_cross_entropy = mean over B of sum over N of the cross entropy against labels (B,N) int64 (recon_fit_behave.py:318-320),
 * C <= 16.  workspace: chore_fit_point_terms_workspace_bytes(B, N).  Backward: up_* device scalars (NULL = 0) -> ddf (B,2,N)
 * (the other channel zero) and dlogits (B,C,N). */
size_t chore_fit_point_terms_workspace_bytes(int B, int N);
int chore_fit_point_terms_fwd(chore_handle* h, const float* df, int channel, float clamp_max, const float* logits,
                              const int64_t* labels, int B, int N, int C, float* out_clamped_mean, float* out_cross_entropy,
                              void* workspace, chore_stream_t stream);
int chore_fit_point_terms_bwd(chore_handle* h, const float* df, int channel, float clamp_max, const float* logits,
                              const int64_t* labels, int B, int N, int C, const float* up_clamped_mean,
                              const float* up_cross_entropy, float* ddf, float* dlogits, chore_stream_t stream);
/* Object side of forward_step (recon_fit_behave.py:165-186).  chore_fit_obj_transform: out (B,N,3) = (verts (B,N,3) R (B,3,3)
 * + t (B,3)) * s (B)  (transform_obj_verts, recon_fit_base.py:367-371); backward: g (B,N,3) -> dR, dt, ds (no gradient for
 * the template points).  chore_fit_obj_terms: out_scale = mean_b (s - scale0)^2 and out_ocent = mean_b sum_k (mean_n
 * object[b,n,k] - (smpl_center[b,k] + mean_n centers[b,3+k,n]))^2 with centers (B,6,N); `diff` (B,3) carries the bracket to
 * the backward, which writes dobject (B,N,3), dcenters (B,6,N) and dscale (B) completely (up_*: device scalars, NULL = 0). */
int chore_fit_obj_transform_fwd(chore_handle* h, const float* verts, const float* R, const float* t, const float* s, int B, int N,
                                float* out, chore_stream_t stream);
int chore_fit_obj_transform_bwd(chore_handle* h, const float* verts, const float* R, const float* t, const float* s, const float* g,
                                int B, int N, float* dR, float* dt, float* ds, chore_stream_t stream);
size_t chore_fit_obj_terms_workspace_bytes(int B);
int chore_fit_obj_terms_fwd(chore_handle* h, const float* object, const float* centers, const float* smpl_center, const float* obj_s,
                            float scale0, int B, int N, float* diff, float* out_scale, float* out_ocent, void* workspace,
                            chore_stream_t stream);
int chore_fit_obj_terms_bwd(chore_handle* h, const float* diff, const float* obj_s, float scale0, const float* up_scale,
                            const float* up_ocent, int B, int N, float* dobject, float* dcenters, float* dscale,
                            chore_stream_t stream);
/* the perturbation of the raw rotation parameter of a step (ReconFitterBase.decopose_axis, recon/recon_fit_base.py:374-384:
 * rot + 1e-4 * U[0,1)), with the draws of all steps laid out up front: out (B,3,3) = rot + scale * noise[*k] with noise
 * (steps,B,3,3), then *k += 1 (k: device int64, the step counter a recorded graph advances; clamped into [0, steps)) */
int chore_fit_rot_noise(chore_handle* h, const float* rot, const float* noise, int64_t* k, float scale, int B, int64_t steps,
                        float* out, chore_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Exact unsigned distance from points to a triangle mesh; its gradient is chore_mesh_dist_bwd below  (what the training-data sampler takes from
 * np.abs(igl.signed_distance(P, V, F)[0]), its I and C, and from trimesh.proximity.ProximityQuery(mesh).vertex(P)[1]:
 * preprocess/boundary_sampler.py:45-64).  points (B,N,3), verts (B,V,3) fp32, faces (F,3) int32 shared by the batch.
 *   dist (B,N)        Euclidean distance to the triangle SURFACE of mesh b: the minimum over all F triangles (interior, edge
 *                     and vertex regions), brute force, no approximation
 *   face_idx (B,N)    a triangle that attains it: smallest fp32 squared distance, then smallest face index; NULL = not wanted
 *   closest (B,N,3)   the closest point on that triangle; NULL = not wanted
 *   vert_idx (B,N)    the nearest mesh VERTEX: smallest fp32 squared distance, then smallest index; NULL = not wanted
 * A zero-area triangle counts as the segment or point it degenerates to; finite inputs give finite outputs.  The optional
 * outputs do not change the bits of the others.  chore_mesh_dist_workspace_bytes depends on the shapes only (0 = unsupported
 * shape); nothing is allocated and no device value is read by the host, so the call can be captured into a graph.
 * ------------------------------------------------------------------------------------------- */
size_t chore_mesh_dist_workspace_bytes(int B, int N, int V, int F);
int chore_mesh_dist_fwd(chore_handle* h, const float* points, const float* verts, const int* faces, int B, int N, int V, int F,
                        float* dist, int* face_idx, float* closest, int* vert_idx, void* workspace, chore_stream_t stream);
/* chore_mesh_dist_fwd plus the side of the surface (no gradient through the winding number): the same dist / face_idx / closest / vert_idx, bit for bit, and
 *   winding (B,N)     the generalized winding number of mesh b about the point (Jacobson et al. 2013): the sum over all F
 *                     triangles of the signed solid angle 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|), a, b, c
 *                     = corners minus the point, divided by 4 pi.  +1 inside a closed mesh whose faces are oriented outward, -1
 *                     where they are oriented inward, 0 outside, fractional about an open mesh; required
 * A triangle of zero area (repeated index, exactly parallel edges) and a point on one of a triangle's corners contribute
 * exactly 0; a point ON the surface gets a finite value whose sign is not specified.  fp32, summed in a fixed order without
 * atomics: the same shapes and inputs give the same bits.  chore_mesh_sdf_workspace_bytes is chore_mesh_dist_workspace_bytes
 * plus the partial sums (0 = unsupported shape); the call can be captured into a graph. */
size_t chore_mesh_sdf_workspace_bytes(int B, int N, int V, int F);
int chore_mesh_sdf_fwd(chore_handle* h, const float* points, const float* verts, const int* faces, int B, int N, int V, int F,
                       float* dist, int* face_idx, float* closest, int* vert_idx, float* winding, void* workspace,
                       chore_stream_t stream);
/* The gradient of dist with respect to the points and the mesh vertices.  face_idx (B,N), closest (B,N,3) and dist (B,N) are
 * the forward's outputs for these very points / verts / faces, g_dist (B,N) the upstream gradient of dist.  `closest` is
 * accepted and NOT read (NULL is allowed): c is formed again in fp64 from the saved winner, because the fp32 rounding of a
 * stored closest point, eps |c|, would enter the direction as eps |c| / dist.  With r = p - c and dist in the sense of |r|:
 *   dpoints (B,N,3)   dpoints[b,n] = g r / |r|, and 0 where dist == 0; NULL = not wanted
 *   dverts (B,V,3)    dverts[b,v] = the sum over all (n,k) with faces[face_idx[b,n]][k] == v of -b_k dpoints[b,n]; NULL = not wanted
 * b_k are the barycentric coordinates of the closest point in its triangle, recomputed here for the saved winner face_idx (the
 * closest point of p on that triangle by its Voronoi regions, in fp64: a point beyond a corner gives the other two corners
 * exactly 0; in the vertex, edge and interior regions alike the derivative with respect to corner k is -b_k r / dist, dist
 * being a minimum over b), clamped to [0,1] with b_0 = 1 - b_1 - b_2.  A vertex that no winning triangle references gets exactly 0.  A zero-area winning triangle
 * gets finite weights that sum to 1 -- nothing more is promised there: the distance is not differentiable in the corners of a
 * degenerate triangle; nor is it where two triangles with different closest points tie (the gradient of the winner is given).
 * A NULL output skips its kernels and does not change the other's bits (as chore_contact_bwd).  The sums over the points are
 * formed per vertex in ascending point order, in chunks whose number depends on the shapes only, without atomics: the same shapes
 * and inputs give the same bits.  chore_mesh_dist_bwd_workspace_bytes depends on the shapes only (0 = unsupported shape); nothing
 * is allocated and no device value is read by the host, so the call can be captured into a graph.  The gradient of the sign-mode
 * "inside" signed distance is this one with g negated where the point is inside (the sign is locally constant); the winding
 * number itself is not differentiated. */
size_t chore_mesh_dist_bwd_workspace_bytes(int B, int N, int V, int F);
int chore_mesh_dist_bwd(chore_handle* h, const float* points, const float* verts, const int* faces, const int* face_idx,
                        const float* closest, const float* dist, const float* g_dist, int B, int N, int V, int F, float* dpoints,
                        float* dverts, void* workspace, chore_stream_t stream);

/* debug aid: with CHORE_NAN_CHECK=1 in the environment chore_query_fwd / chore_query_bwd_points scan their inputs and
 * outputs for non-finite values (extra launches on the caller's stream); out32[0..15] = counts per site (0 points, 1-4 the
 * forward's df / pca / parts / centers, 5 / 6 the maps, 8 points, 9-12 the upstream gradients, 13 dpoints), out32[16..31] =
 * sequence number of the first scan of that site that saw one */
int chore_debug_nan_counts(unsigned* out32);
/* debug aid: what the last convolution launch on the handle (chore_conv2d_fwd, chore_conv2d_bwd_data, every layer of the encoder
 * and of the training operators) chose.  Writes min(n, 8) ints and returns that count (negative: bad argument):
 *   out[0] kernel family: 1 conv_lds_kernel, 2 conv_small_kernel, 3 conv_pc_kernel, 4 conv_mw_kernel, 5 conv_rw_kernel (0: none yet)
 *   out[1] rows of a tile (conv_small_kernel: rows per workgroup; conv_rw_kernel: 0)   out[2] output channels per workgroup
 *   out[3] taps per K-step   out[4] K-steps of weights resident in LDS (0 where the kernel has no such ring)
 *   out[5] flags: 1 scaled-input variant (data gradient of CHORE_F16X3), 2 GroupNorm fused into the input, 4 small-grid variant
 *          of conv_lds_kernel, 8 residual added in the epilogue, 16 pooled output written by the epilogue
 *   out[6] input channels   out[7] convolution launches on the handle so far
 * Host stores only: no kernel and no result changes. */
int chore_debug_last_conv(chore_handle* h, int* out, int n);
/* debug aid: what the last weight-gradient launch on the handle (chore_conv2d_bwd_weight, chore_gemm_tn_f32, every layer of
 * chore_convblock_bwd) chose.  Writes min(n, 8) ints and returns that count (negative: bad argument):
 *   out[0] kernel: 1 wgrad_kernel (32-channel tiles), 2 wgrad64_kernel, 3 wgrad64_x3_kernel, 4 wgrad64_x3_pc_kernel,
 *          5 wgrad128_x3_pc_kernel (0: none yet)
 *   out[1] element type of the arithmetic: CHORE_F32, CHORE_BF16 or CHORE_F16X3 (a CHORE_F16X3 layer below 64 channels reports
 *          CHORE_F32: it runs the fp32 kernel)
 *   out[2] taps   out[3] channels per tile side   out[4] shares S of the pixel tiles   out[5] pixel tiles
 *   out[6] flags: 1 GroupNorm + ReLU recomputed on the input, 2 dbias requested, 4 the XCD-interleaved workgroup -> (share,
 *          channel pair) mapping (S % 8 == 0 in the 64- and 128-channel kernels) instead of the linear one
 *   out[7] weight-gradient launches on the handle so far
 * Host stores only: no kernel and no result changes. */
int chore_debug_last_wgrad(chore_handle* h, int* out, int n);
/* which kernel a query call runs (csrc/query_plan.h; no handle, no device): what the entry point decides for these arguments.
 *   op         0 chore_query_fwd[_ws], 1 chore_query_fwd_train, 2 chore_query_bwd_points, 3 chore_gen_surface_step_fused,
 *              4 chore_query_bwd_train
 *   dtype      as the entry point takes it, CHORE_HEADS_X3 included     B, N, FH, FW  as there (the other map never matters)
 *   live_mask  op 2: bit 0 g_df, bit 1 g_parts, bit 2 g_pca, bit 3 g_centers is not NULL
 *   flags      bit 0: a workspace is passed (op 0), bit 1: have_forward (op 4)
 *   switches   bit 0 CHORE_QUERY_W4, bit 1 CHORE_QUERY_X3_NOSPLIT, bit 2 CHORE_QUERY_NO_ONE_HEAD; -1: this process's
 *              environment, as the entry points read it -- once, before their first call
 * Writes min(n, 9) ints and returns that count, or CHORE_EINVAL for a bad argument and for what the entry point refuses (fp16
 * maps in training, fp16 x 3 training backward without the staged forward, a surface step without the fp16 x 3 heads):
 *   out[0] kernel: 0 query_fwd_x3_split_kernel, 1 query_fwd_f32_kernel, 2 query_fwd_f32_w8_kernel, 3 query_bwd_f32_kernel
 *   out[1] the template's NCB (1 in the eight-wave kernels)   out[2] waves of a workgroup (the template's NW: 4 or 8)
 *   out[3] template flags: 1 TRAIN, 2 STAGED, 4 X3 (heads on the fp16 matrix cores), 8 SURF, 16 ONE
 *   out[4] ONE without SURF: the head that has the gradient (0 df, 1 parts, 2 pca, 3 centers)
 *   out[5] points of a tile   out[6] threads of a workgroup   out[7] 1: the sort runs first (query_bin_kernel, query_perm_kernel)
 *   out[8] the kernel's T: the maps' type (CHORE_F32 float, CHORE_BF16 unsigned short, CHORE_F16 qh16_t) */
int chore_query_plan(int op, int dtype, int B, int N, int FH, int FW, int live_mask, int flags, int switches, int* out, int n);
/* which kernel and tiling a forward / data-gradient convolution launch gets (csrc/conv_plan.h; no handle, no device): what launch_conv
 * decides for these arguments under this process's switches (CHORE_CONV_*, CHORE_NO_CONV_SMALL, CHORE_PC_FORCE: read once per process).
 *   dtype, taps (1 | 9), B, H, W, Cin, Cout   the launch's mode and shape (Cin, Cout: of the launched convolution)
 *   traits_bits  1 GroupNorm fused into the input, 2 scaled operand (the data gradient of CHORE_F16X3), 4 residual, 8 second residual,
 *                16 pooled output, 32 `out` is written
 *   fill         0, or 128 as the inference encoder asks (the least number of workgroups a small layer's tiling must yield)
 * Writes min(n, 7) ints and returns that count, or CHORE_EINVAL for a bad argument and for what launch_conv refuses:
 *   out[0..5]    as chore_debug_last_conv: kernel family, rows, channels per workgroup, taps per K-step, resident K-steps, flags
 *   out[6]       the profile class of the launch in the encoder: the index among the conv_* classes of chore_profile_read */
int chore_conv_plan(int dtype, int taps, int B, int H, int W, int Cin, int Cout, int traits_bits, int fill, int* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* CHORE_HIP_H */
