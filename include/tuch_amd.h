/*
 * libtuch_amd -- MI355X (gfx950) implementation of TUCH's self-contact path.
 *
 * C ABI: plain device pointers and sizes, one HIP stream per call, no torch types.
 * The reference (muelea/tuch) is pure Python with no FFI layer; every entry point
 * below replaces the reference function(s) cited next to it and is what a binding
 * for that function would call (INTEGRATION.md shows the ctypes stubs).
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless marked "host"; float = IEEE binary32;
 *     tensors are dense row-major with the shape given in the comment
 *   - return 0 on success, negative on failure; tuch_last_error() describes the last
 *     failure on the calling thread; nothing is thrown across the ABI
 *   - hot calls never allocate, never synchronise and are hipGraph-capturable; scratch
 *     memory is passed in by the caller (size from the matching *_workspace_bytes)
 *   - `stream` is a hipStream_t (NULL = default stream)
 *   - results are deterministic (fixed reduction order); only gradient scatters use
 *     float atomics
 */
#ifndef TUCH_AMD_H
#define TUCH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* tuch_last_error(void);
/* 2.  Since 1: one entry point per operation -- the superseded stage-2, nearest-vertex and body-model forms are gone,
 * tuch_v2v_min_model, tuch_smpl_backward_split and tuch_smplify_stage2_fused take the argument lists given below. */
int tuch_abi_version(void);

/* per-model constants, see tuch_contact_model_create below */
typedef struct tuch_contact_model tuch_contact_model;

/* ---- tuch/utils/contact.py ------------------------------------------------------- */

/* batch_pairwise_dist(x, y, use_cuda, squared), contact.py:23-47.
 * x [B,Nx,3], y [B,Ny,3] -> P [B,Nx,Ny] = |x|^2 + |y|^2 - 2 x.y (sqrt of it if !squared).
 * Materialising form kept for API parity; the hot path uses tuch_v2v_min_masked. */
int tuch_batch_pairwise_dist(const float* x, const float* y, int B, int Nx, int Ny, int squared,
                             float* P, void* stream);

/* Adjoint of batch_pairwise_dist for callers that differentiate through the matrix (the reference does:
 * tuch/smplify/losses.py:76-78 -> 115-116, tuch/eft/loss.py:142; torch autograd through the three bmm of
 * contact.py:27-29).  grad_P [B,Nx,Ny] -> grad_x [B,Nx,3] and/or grad_y [B,Ny,3] (either may be NULL):
 * grad_x_i = 2 sum_j g_ij (x_i - y_j), grad_y_j = 2 sum_i g_ij (y_j - x_i); !squared: g / (2 sqrt(P)) first.
 * Fixed summation order (no atomics). */
int tuch_batch_pairwise_dist_bwd(const float* x, const float* y, const float* grad_P, int B, int Nx, int Ny,
                                 int squared, float* grad_x, float* grad_y, void* stream);

/* Adjoint of solid_angles / winding_numbers for callers that differentiate through them (plain torch ops in the reference,
 * contact.py:79-109,147; the reference itself only calls them under torch.no_grad()).  grad_out [B,Q,F] (adjoint of
 * tuch_solid_angles) or grad_w [B,Q] (of tuch_winding_numbers), exactly one; grad_points [B,Q,3] and / or grad_triangles
 * [B,F,3,3] (either may be NULL).  torch's conventions at the singular points: d|a|/da = 0 at a = 0, NaN where the query sits
 * on a corner (atan2 at (0,0)).  Fixed summation order. */
int tuch_solid_angles_bwd(const float* points, const float* triangles, const float* grad_out, const float* grad_w,
                          int B, int Q, int F, float* grad_points, float* grad_triangles, void* stream);

/* solid_angles(points, triangles, thresh), contact.py:49-109.
 * points [B,Q,3], triangles [B,F,3,3] -> out [B,Q,F] = 2*atan2(num, den). */
int tuch_solid_angles(const float* points, const float* triangles, int B, int Q, int F, float* out,
                      void* stream);

/* winding_numbers(points, triangles, thresh), contact.py:112-147, fused with the callers'
 * `.le(0.99)` (losses.py:82, loss.py:262,297).  w [B,Q] and/or exterior [B,Q] (1 = w <= thresh);
 * either output may be NULL.  Never materialises anything of size QxF. */
size_t tuch_winding_workspace_bytes(int B, int Q, int F);
int tuch_winding_numbers(const float* points, const float* triangles, int B, int Q, int F, float* w,
                         uint8_t* exterior, float exterior_thresh, void* workspace,
                         size_t workspace_bytes, void* stream);

/* triangles = verts[b][face_tensor[0]], losses.py:81 / loss.py:260.
 * verts [B,V,3], faces [F,3] int32 -> triangles [B,F,3,3]. */
int tuch_gather_triangles(const float* verts, const int32_t* faces, int B, int V, int F,
                          float* triangles, void* stream);

/* ---- masked nearest vertex: losses.py:76-78,92-93 / loss.py:255-257,269-270 -------- */

/* geomask (geod > geothres, smplifydc.py:65 / loss.py:71) as bits: word [w][j] holds
 * columns 64w..64w+63 of row j; tuch_geomask_words(V) words per row set (even, zero padded). */
int tuch_geomask_words(int V);
size_t tuch_geomask_bits_bytes(int V);
int tuch_pack_geomask(const uint8_t* geomask /* [V,V] bytes */, int V, uint64_t* bits, void* stream);

/* For every column i: min / argmin over rows j with geomask[j][i] of |v_i - v_j|^2
 * (first index on ties, all-masked -> (inf, 0), as torch.min / torch.argmin).
 * points [B,N,3], bits from tuch_pack_geomask or a model -> min_d2 [B,N], argmin [B,N] int32. */
size_t tuch_v2v_workspace_bytes(int B, int N);
int tuch_v2v_min_masked(const float* points, const uint64_t* geomask_bits, int B, int N, float* min_d2,
                        int32_t* argmin, void* workspace, size_t workspace_bytes, void* stream);

/* Ragged variant for the HD resampling of loss.py:284-291: body b owns points
 * offsets[b]..offsets[b+1] (device int32 [B+1]); point a inherits the mask row/column of template
 * vertex vertex_ids[a] (geovec_verts, loss.py:88).  argmin is relative to the body's first point (first index
 * among equal minima, 0 when no row is admissible).  Rows are visited in chunks of 32 that are skipped when
 * their bounding box is farther than the columns' current minima: any point order is exact, points of a body
 * that are sorted by surface patch are fast. */
size_t tuch_v2v_min_indexed_workspace_bytes(int B, int max_points_per_body);
int tuch_v2v_min_indexed(const float* points, const int32_t* vertex_ids, const int32_t* offsets,
                         const uint64_t* geomask_bits, int B, int V, int max_points_per_body, float* min_d2,
                         int32_t* argmin, void* workspace, size_t workspace_bytes, void* stream);
/* The same search on the matrix cores (what the HD branch of tuch_hd_contact_fwd runs by default): distances of 32 rows x
 * 64 columns from v_mfma_f32_32x32x2_f32 in coordinates relative to the column block, the mask as a bf16 penalty product.
 * The winner of a column is the row with the smallest 20-bit key of that distance: it may differ from
 * tuch_v2v_min_indexed's between rows whose squared distances tie within ~1e-6 relative + a few ulp of the block's
 * squared radius (the reference's own |x|^2+|y|^2-2x.y form is noisier); min_d2 is the direct-difference distance of
 * the winner.  Same arguments. */
size_t tuch_v2v_min_indexed_mfma_workspace_bytes(int B, int max_points_per_body);
int tuch_v2v_min_indexed_mfma(const float* points, const int32_t* vertex_ids, const int32_t* offsets,
                              const uint64_t* geomask_bits, int B, int V, int max_points_per_body, float* min_d2,
                              int32_t* argmin, void* workspace, size_t workspace_bytes, void* stream);

/* ---- pull/push terms: losses.py:96-105 (mode 0) / loss.py:303-315 (mode 1) ---------- */

/* terms [B,2] = (sum over interior, sum over exterior) of weight*tanh(d/scale)^2 with
 * d_i = |x_i - x_partner(i)|; body_valid [B] bytes or NULL (invalid bodies give 0). */
int tuch_contact_terms_fwd(const float* points, const int32_t* partner, const uint8_t* exterior,
                           const uint8_t* body_valid, int B, int N, int mode, float euclthres,
                           float* terms, void* stream);
/* Ragged forward (HD points, loss.py:299-315): body b owns points offsets[b]..offsets[b+1] of one
 * concatenated set [N,3]; partner holds global indices; terms [B,2]. */
int tuch_contact_terms_ragged_fwd(const float* points, const int32_t* partner, const uint8_t* exterior,
                                  const int32_t* offsets, int B, int mode, float euclthres, float* terms,
                                  void* stream);
int tuch_contact_terms_ragged_bwd(const float* points, const int32_t* partner, const uint8_t* exterior,
                                  const int32_t* body_of_point, const float* grad_scale, int N, int mode,
                                  float euclthres, float* grad_points, void* stream);
/* grad_points [B,N,3] += d(terms)/d(points) . grad_scale [B,2]; grad_points zeroed by the caller. */
int tuch_contact_terms_bwd(const float* points, const int32_t* partner, const uint8_t* exterior,
                           const float* grad_scale, int B, int N, int mode, float euclthres,
                           float* grad_points, void* stream);
/* The same scatter in deterministic mode (tuch_set_deterministic): grad_fixed_zeroed = B*N*3 zeroed 64-bit words the
 * contributions are added to as fixed-point integers (order-independent), then converted: grad_points is WRITTEN
 * (no need to clear it), bit-reproducible.  Valid range as for tuch_smplify_stage2_fused. */
int tuch_contact_terms_bwd_fixed(const float* points, const int32_t* partner, const uint8_t* exterior,
                                 const float* grad_scale, int B, int N, int mode, float euclthres,
                                 void* grad_fixed_zeroed, float* grad_points, void* stream);

/* RegressorLoss.contact_loss's last line, loss.py:317 (`loss_contact.sum() / valid_fit.sum()` over the per-body terms of
 * :272 / :315): terms [B,K] summed over the bodies with valid[b] != 0 and divided by their number, in one launch.
 * out [2] = (mean, 1 / number of valid bodies); no valid body: 0 / 0 = NaN, as the reference's division.
 * Backward: grad_terms [B,K] = upstream[0] * (valid[b] ? out[1] : 0) -- what tuch_contact_terms_bwd takes as grad_scale. */
int tuch_valid_mean_fwd(const float* terms, const uint8_t* valid, int B, int K, float* out, void* stream);
int tuch_valid_mean_bwd(const float* upstream, const float* fwd_out, const uint8_t* valid, int B, int K,
                        float* grad_terms, void* stream);

/* Reprojection + pose-prior part of the SMPLify-DC objective, losses.py:56-64 (projection
 * geometry.py:83-111 with identity rotation, gmof losses.py:25-32, max-mixture prior
 * prior.py:117-132).  out [B,2] = (sum_j conf^2 gmof, prior_scale * prior); gradients for a unit
 * upstream gradient.  body_pose may be NULL (no prior). */
int tuch_smplify_small_terms(const float* joints, const float* camera_t, const float* camera_center,
                             const float* joints_2d, const float* joints_conf, const float* body_pose,
                             const float* gmm_means, const float* gmm_precisions, const float* gmm_log_weights,
                             int B, int num_joints, int num_gaussians, float focal_length, float sigma,
                             float prior_scale, float* out, float* grad_joints, float* grad_camera_t,
                             float* grad_body_pose, void* stream);

/* The stage-1 objective of SMPLify-DC, camera_fitting_loss (tuch/smplify/losses.py:125-152), in one launch:
 * out[0] = sum_b [ sum_j conf^2 gmof(proj - j2d, sigma) + depth_weight^2 (t_z - t_z^est)^2 + shape_weight^2 |betas_b|^2 ]
 * and its gradients for a unit upstream gradient: grad_joints [B,J,3], grad_camera_t [B,3], grad_betas [B,num_betas]
 * (betas / grad_betas may be NULL: no shape term).  share: B floats of scratch; ticket: one int, zero before the first
 * call and left zero by every call (the block that arrives last adds the bodies up in body order: deterministic). */
int tuch_smplify_stage1_terms(const float* joints, const float* camera_t, const float* camera_t_est,
                              const float* camera_center, const float* joints_2d, const float* joints_conf,
                              const float* betas, int B, int num_joints, int num_betas, float focal_length, float sigma,
                              float depth_weight, float shape_weight, float* share, int* ticket, float* out,
                              float* grad_joints, float* grad_camera_t, float* grad_betas, void* stream);

/* Adam update (torch.optim.Adam without weight decay / amsgrad: tuch/smplify/smplifydc.py:117,150 optimises body pose,
 * global orientation, betas, camera translation with it) of up to 8 small tensors in ONE launch, the step counter on the
 * device (capturable).  params / grads / exp_avg / exp_avg_sq: `count` device pointers each (host arrays), sizes[k]
 * floats; betas [count][2]; step: one device float = updates so far, incremented by the call. */
int tuch_adam_step(int count, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const int* sizes, const float* betas, float* step, float lr, float eps,
                   void* stream);

/* ---- tuch/utils/smplxtosmpl_mtp.py: fitting the body model to target meshes in correspondence ------------------ */

/* The data term of one iteration (:100-101) in one launch.  verts, target [B,V,3], transl [B,3], weights [V] or NULL
 * (all ones: the reference's term), weight_sum = sum_v w_v (V without weights; never 0):
 *   d_v = verts_v + transl - target_v,   loss[b] = sum_v w_v |d_v| / weight_sum,   total[0] = sum_b loss[b]
 * and the gradients of total for a unit upstream gradient: grad_verts [B,V,3] = w_v d_v / (|d_v| weight_sum) -- a zero
 * row where |d_v| = 0 (torch.norm's convention) and where w_v = 0 (such a vertex is not read: its target may be
 * non-finite) -- and grad_transl [B,3] = sum_v grad_verts.  The four per-body sums and the total are fixed-order sums,
 * the same bits on every call in either mode of tuch_set_deterministic.  scratch: tuch_vertex_fit_scratch_floats(B, V)
 * floats; ticket: one int, zero before the first call and left zero by every call. */
size_t tuch_vertex_fit_scratch_floats(int B, int V);
int tuch_vertex_fit_terms(const float* verts, const float* transl, const float* target, const float* weights, int B,
                          int V, float weight_sum, float* scratch, int* ticket, float* loss, float* total,
                          float* grad_verts, float* grad_transl, void* stream);

/* out[b,i,:] = sum_k data[k] src[b, indices[k], :] over the CSR row k in [indptr[i], indptr[i+1]) (:58 with the
 * [6890 x 10475] SMPL-X -> SMPL matrix).  src [B,num_src,3] -> out [B,num_rows,3]; indptr [num_rows+1] int32, indices
 * int32 in [0, num_src) -- the CALLER checks the range when it builds the table --, data float32.  A row's entries are
 * added in float32 in the order they are stored (deterministic); a row may hold any number, none gives zeros. */
int tuch_mesh_transfer(const int* indptr, const int* indices, const float* data, const float* src, int B, int num_rows,
                       int num_src, float* out, void* stream);

/* Objective assembly of losses.py:120-123 as one deterministic reduction:
 * out[0] = sum(small_terms [B,2]) + contact_scale * sum(contact_terms [B,2]) + r2r_scale * sum(r2r [B,P]). */
int tuch_smplify_objective(const float* small_terms, const float* contact_terms, const float* r2r, int B, int P,
                           float contact_scale, float r2r_scale, float* out, void* stream);
int tuch_smplify_objective_bwd(const float* grad_out, int B, int P, float contact_scale, float r2r_scale,
                               float* grad_small, float* grad_contact, float* grad_r2r, void* stream);

/* The tail of the stage-2 objective (tuch/smplify/losses.py:96-123) and its vertex gradient in one launch:
 *   out[0] = sum_b [ small_terms[b,0] + small_terms[b,1] + contact_scale (interior_b + exterior_b) + r2r_scale sum_p d2[b,p] ]
 * with the contact sums of tuch_contact_terms_fwd (0 for bodies with body_valid == 0; body_valid may be NULL) and d2 the
 * region pairs' minima, decoded from pair_keys [B,P] (tuch_region_pair_keys of `model`; P = 0: NULL, no region term).
 * The objective is the root of the fit's autograd graph, so the gradient for a UNIT upstream gradient is scattered while
 * the sums are formed: into grad_points [B,N,3] (float atomics, pre-zeroed) or into grad_fixed_zeroed (deterministic
 * mode, below); give at most one of the two, neither: the value alone.  out[0] is a fixed-order sum, the same bits in all
 * three cases.  share: tuch_smplify_stage2_fused_scratch_floats(B) floats; ticket: one int, zero before the call, left
 * zero.  The unit gradients of the small terms are tuch_smplify_small_terms' own outputs. */
size_t tuch_smplify_stage2_fused_scratch_floats(int B);
int tuch_smplify_stage2_fused(const float* points, const int32_t* partner, const uint8_t* exterior,
                              const uint8_t* body_valid, int B, int N, int mode, float euclthres,
                              const float* small_terms, int P, float contact_scale, float r2r_scale, float* share,
                              int* ticket, float* out, float* grad_points, const tuch_contact_model* model,
                              const void* pair_keys, void* grad_fixed_zeroed, void* stream);
/* Deterministic mode -- ON by default (TUCH_DETERMINISTIC=0 in the environment when the library is loaded, or
 * tuch_set_deterministic(0), selects float atomics: last-ulp run-to-run noise in the gradients): the gradient scatters of
 * tuch_smplify_stage2_fused (contact terms, region minima) and of tuch_smpl_backward_split (skinning adjoint) accumulate 64-bit
 * fixed-point numbers (2^-36) with integer atomics instead of floats -- sums that do not depend on the order of arrival,
 * so an SMPLify-DC fit reproduces bit for bit.  tuch_smplify_stage2_fused then wants grad_fixed_zeroed = B*N*3 zeroed
 * 64-bit words (NULL: float atomics, whatever the mode): the accumulators are the result, read as they are by
 * g_verts_fixed of tuch_smpl_backward_split or converted by tuch_fixed_to_float.
 * VALID RANGE of the fixed-point sums: |sum| < 2^27 = 1.3e8 (beyond, the unsigned 64-bit accumulator wraps silently) and
 * contributions below 2^-37 = 7e-12 round to zero.  Gradient magnitudes scale with contact_scale / r2r_scale: with the
 * reference's weights (10, 2000) and metre-scale bodies the per-vertex gradients are < 1e5. */
/* n fixed-point sums -> floats */
int tuch_fixed_to_float(const void* fixed, size_t n, float* out, void* stream);
void tuch_set_deterministic(int on);
int tuch_get_deterministic(void);

/* The region-pair search of tuch_region_pair_min alone, for tuch_smplify_stage2_fused(model, pair_keys): keys [B,P]
 * 64-bit words, ZERO on entry (the caller clears them with whatever else it clears); no clearing and no finalize
 * launch. */
int tuch_region_pair_keys(const tuch_contact_model* model, const float* verts, int B, const uint8_t* select,
                          int use_geomask, void* keys_zeroed, void* stream);

/* ---- per-model constants -------------------------------------------------------------
 * Host tables in, device copies kept by the handle.  Segments follow
 * tuch/utils/segmentation.py:29-99: seg_q = segment_vidx lists; seg_faces = faces of the
 * closed segment where cap vertex c (global numbering over all segments) has index V + c;
 * cap_* = the ordered boundary loops whose mean is the cap vertex.  Regions follow
 * ContactSigSMPL / classes (train_module.py:64-66): CSR vertex lists and [P,2] pairs. */
int tuch_contact_model_create(tuch_contact_model** out, int V, int F, const int32_t* faces /* host [F,3] */,
                              const uint8_t* geomask /* host [V,V] bytes or NULL */,
                              int num_segments, const int32_t* seg_q_off, const int32_t* seg_q_vidx,
                              const int32_t* seg_f_off, const int32_t* seg_faces,
                              int num_caps, const int32_t* cap_off, const int32_t* cap_vidx,
                              int num_regions, const int32_t* region_off, const int32_t* region_vidx,
                              int num_pairs, const int32_t* pairs);
void tuch_contact_model_destroy(tuch_contact_model* model);
/* Switches of the hot calls (A/B measurements, tests): winding_ray (0 never / 1 when only flags are wanted / 2 also for
 * w), winding_tree, tree_waves, ray_pair_cap, ray_waves, v2v_tree, v2v_pairs, v2v_waves,
 * seg_splits, seg_fused, seg_assist (fixed at create), hd_search, hd_search_waves, hd_overlap, canary.  (Deterministic mode is process-wide: tuch_set_deterministic.)  The environment variables TUCH_<NAME> are read ONCE, by
 * tuch_contact_model_create; afterwards only set_option changes a model's switches -- no hot call looks at the
 * environment, so a captured hipGraph cannot depend on it.  (The workspace sizes depend on ray_pair_cap and canary:
 * query *_workspace_bytes again after changing them.)
 * hd_search_waves (wavefronts per block of 64 columns in the matrix-core search of the HD branch) has three forms, 4, 2
 * and 1; any other value is accepted and mapped silently: >= 4 runs the form with 4, 2 or 3 the form with 2, anything
 * below 2 (0 and negative values included) the form with 1.  get_option returns the value as it was set. */
int tuch_contact_model_set_option(tuch_contact_model* model, const char* name, int value);
int tuch_contact_model_get_option(const tuch_contact_model* model, const char* name, int* value);
/* Option canary = 1 (debug): every region of every workspace of the model's hot calls (nearest-vertex search, inside
 * test incl. its pair lists, winding of points, the HD branch's worst-case buffers and saved state) is followed by 256
 * guard bytes, written with 0xDEADBEEF before the call's kernels and compared after them, on the call's stream.
 * canary_hits: guard words found changed since the last reset (synchronises the device).  selftest: arms three regions
 * in `workspace` (>= 4 KiB), overruns one by a word on purpose and returns the number of hits counted (1). */
int tuch_contact_model_canary_hits(const tuch_contact_model* model, int* hits_host, int reset);
int tuch_contact_model_canary_selftest(const tuch_contact_model* model, void* workspace, size_t workspace_bytes, void* stream);
const uint64_t* tuch_contact_model_mask_bits(const tuch_contact_model* model);
/* The geodesic mask packed in the cluster tree's vertex order (device, same layout as mask_bits with vertex v
 * replaced by its position in tuch_cluster_tree_export's qperm), or NULL without tree or mask: neighbouring
 * positions are neighbours on the surface, so a wavefront of nearby points touches few mask words. */
const uint64_t* tuch_contact_model_tree_mask_bits(const tuch_contact_model* model);
int tuch_contact_model_info(const tuch_contact_model* model, int* V, int* F, int* num_segments,
                            int* seg_q_total, int* num_pairs);
/* The triangle-strip walk of the faces used by the winding kernel (inspection / tests):
 * stream_len vertex ids with sign 0 (prime) or +-1 (emit triangle of the last three ids). */
int tuch_contact_model_strips(const tuch_contact_model* model, int* stream_len, int* num_strips,
                              int32_t* vidx_host, float* sign_host);

/* Measurement aid for the hierarchical winding numbers inside tuch_exterior_flags: walks the cluster tree
 * for verts [B,V,3] and reports the stream elements the wavefronts stepped through.  out_host[4] =
 * {leaf-strip elements, cap elements, wavefronts, elements of the flat strip stream}; one element step
 * serves 64 queries (one wavefront).  Workspace as for tuch_exterior_flags.  Synchronises the stream. */
int tuch_winding_tree_work(const tuch_contact_model* model, const float* verts, int B, void* workspace,
                           size_t workspace_bytes, unsigned long long* out_host, void* stream);

/* Measurement aid for the ray-crossing inside test (csrc/ray_winding.hip) that tuch_exterior_flags and
 * tuch_winding_points use when only the flags are wanted: out_host[4] = {strip elements stepped through by all
 * passes, (ray, element) pairs whose ray passes the slabs of the element's leaf, 64 x elements listed, passes}: [1] /
 * [2] is the share of lanes that can have a crossing at all.  A pass is one wavefront's walk of one leaf's strip for one
 * tile of that leaf's rays, counted over all B bodies: a leaf with c >= 64 rays has c / 64 tiles, the last of which
 * carries the c % 64 rays left over as a second ray set of the same pass; a leaf with 0 < c < 64 rays has one.  [0]
 * counts a pass's strip once, whether the pass holds one ray set or two (a second set filters the strip once more
 * without fetching or staging it again).  Workspace as for tuch_exterior_flags.  Synchronises the stream. */
int tuch_ray_work(const tuch_contact_model* model, const float* verts, int B, void* workspace,
                  size_t workspace_bytes, unsigned long long* out_host, void* stream);
/* FOR THE TESTS ONLY (tests/test_near_encode.py, tests/test_gpu_near_lists.py): the numbers and the lists of the inside
 * test's near stage (csrc/ray_winding.hip: ray_leaf_bounds_kernel, ray_near_kernel).
 * tuch_near_encode_host runs the kernels' own conversion of a single-precision value to the near test's signed 16-bit
 * fixed point on the HOST (no GPU needed): round_up != 0 the smallest level >= value, otherwise the largest level <= value,
 * saturating (NaN: +32767 rounding up, -32768 rounding down).  *out = the level, value * 8192 rounded. */
int tuch_near_encode_host(float value, int round_up, int* out);
/* tuch_ray_near_debug runs the two kernels as a call of tuch_exterior_flags (points == NULL: the model's vertices) or of
 * tuch_winding_points (points [B,Q,3], counts [B] or NULL) does and copies out (device pointers, each may be NULL), with
 * L = dims_host[0] leaves and N = dims_host[1] query blocks of 64 slots:
 *   out_bounds  [B][13][L] float : the padded single-precision bounds as formed before encoding, in the order of the
 *                                  record's halves: lower bounds of the slabs x y x+y x-y x-z y-z, upper bounds of x y z
 *                                  x+y x-y x+z y+z (sheared frame, relative to the body's reference point);
 *   out_records [B][L][8] uint32 : the encoded records (13 halves, the leaf number, the node);
 *   out_rays    [B][N*64][9] float : x y z x+y x-y x+z x-z y+z y-z of every query slot (slots of blocks behind a body's
 *                                  last point are left as they were);
 *   out_bitmap  [B][L][N*8] uint8 : bit (slot & 7) of byte (slot >> 3) set where (leaf, slot) is listed;
 *   out_leaves  [B][N][L] int32  : the leaves of every block's list in list order, -1 behind its end;
 *   out_len     [B][N] int32     : the lists' lengths.
 * waves: 0 the form the step would take for these sizes, 1 / 4 wavefronts per query block.  dims_host[2] = the workspace
 * bytes needed; verts == NULL: only dims_host is filled.  Not on any timed path. */
int tuch_ray_near_debug(const tuch_contact_model* model, const float* verts, const float* points, const int32_t* counts,
                        int B, int Q, int waves, void* workspace, size_t workspace_bytes, long long* dims_host,
                        float* out_bounds, uint32_t* out_records, float* out_rays, uint8_t* out_bitmap,
                        int32_t* out_leaves, int32_t* out_len, void* stream);
/* The cluster tree the model built for itself: qperm_host [V] = vertices in tree order, face_leaf_host [F] = leaf
 * (preorder sequence number) of every face; either may be NULL.  Fails when the model has no tree. */
int tuch_contact_model_tree_order(const tuch_contact_model* model, int32_t* qperm_host, int32_t* face_leaf_host);

/* Model-level form of tuch_v2v_min_masked: uses the model's geodesic mask and, when the model has a
 * cluster tree, a pruned walk that gives the same minima (rows whose posed box is farther than a column's
 * current minimum, or that the mask rules out entirely, are skipped).  Exact ties between rows are
 * resolved deterministically (smallest row in the tree's vertex order). */
size_t tuch_v2v_model_workspace_bytes(const tuch_contact_model* model, int B);
/* hint_inout (optional, tuch_v2v_hint_bytes bytes, device, opaque, zero-initialised by the caller): the partners found
 * by this call are left there and seed the next call with the same buffer -- in an iterative fit the previous
 * iteration's partner is still admissible and almost as close, so nearly every box is pruned at once.  The result
 * does not depend on the hint (any content is safe); only the run time does.  Used only with a cluster tree. */
size_t tuch_v2v_hint_bytes(const tuch_contact_model* model, int B);
/* flags: for callers that run other kernels beside the search on another stream (as ops.ContactModel.exterior_and_partner
 * does with the inside test), TUCH_V2V_LEAVE_ROOM caps the walk's occupancy so that the neighbours' small kernels are not
 * starved of wave slots; TUCH_V2V_NEAR_FINAL: the caller expects hint_inout to hold near-final partners (an iterative
 * fit calling again after a small parameter update) -- the search then uses fewer, longer wavefronts.  Same results
 * whatever the flags.
 * `zero` (16-byte aligned, zero_bytes a multiple of 16; or NULL / 0) is cleared by the call's first kernel: on the stream,
 * before anything the caller enqueues behind the call -- instead of a fill launch of its own (SMPLify-DC stage 2: the
 * vertex gradient its tail scatters into, the tail's arrival counter, the region pairs' keys). */
enum { TUCH_V2V_LEAVE_ROOM = 1, TUCH_V2V_NEAR_FINAL = 2 };
int tuch_v2v_min_model(const tuch_contact_model* model, const float* verts, int B, float* min_d2, int32_t* argmin,
                       void* hint_inout, void* workspace, size_t workspace_bytes, int flags, void* zero, size_t zero_bytes,
                       void* stream);

/* Cluster tree over the faces of a closed mesh (host only, no device needed): the structure behind the
 * hierarchical evaluation of winding_numbers (tuch/utils/contact.py:112-147) inside tuch_exterior_flags.
 * A set of faces far from the query is replaced by a triangulation of its boundary loops, which subtends
 * the same solid angle for every query outside the set's bounding box (exact in real arithmetic).
 * nodes [num_nodes][8] = {cap_off, cap_len, exact_off, exact_len, skip, child0, child1, num_faces} in
 * preorder; vidx / sign [stream_len] = strip stream as in tuch_contact_model_strips (leaf strips in
 * [0, exact_len), then the caps); qperm [num_qblocks*128] = query order; frontier f =
 * frontier_nodes[frontier_off[f] .. frontier_off[f+1]) = subtrees that together cover the mesh;
 * launch_order [frontier_total * num_qblocks] = per frontier (at frontier_off[f] * num_qblocks) the
 * (subtree index << 16 | query block) pairs, the long-running ones first; rows [num_nodes][2] = (first
 * position, count) in qperm of the vertices below a node (each vertex belongs to one leaf); face_leaf [F] =
 * sequence number of the leaf holding each face (sort query points by it to make them coherent).
 * tuch_contact_model_create builds the same tree internally.  Fails (TUCH_ERR_ARG) for a mesh that is
 * not a closed, consistently oriented manifold; the library then keeps the flat evaluation. */
typedef struct tuch_cluster_tree tuch_cluster_tree;
int tuch_cluster_tree_build(int V, int F, const int32_t* faces, int leaf_faces, tuch_cluster_tree** out);
void tuch_cluster_tree_free(tuch_cluster_tree* tree);
int tuch_cluster_tree_info(const tuch_cluster_tree* tree, int* num_nodes, int* exact_len, int* stream_len,
                           int* num_qblocks, int* num_frontiers, int* frontier_total);
int tuch_cluster_tree_export(const tuch_cluster_tree* tree, int32_t* nodes, int32_t* vidx, float* sign,
                             int32_t* qperm, int32_t* frontier_off, int32_t* frontier_nodes,
                             int32_t* launch_order, int32_t* rows, int32_t* face_leaf);

/* exterior flags of losses.py:79-89 / loss.py:259-266: winding_numbers(verts, verts[faces]).le(thresh),
 * then BatchBodySegment.batch_has_self_isec (segmentation.py:117-124) and the re-marking of
 * vertices interior to their own segment.  verts [B,V,3] -> exterior [B,V] bytes;
 * optional: w [B,V], seg_w / seg_exterior [B, seg_q_total]. */
size_t tuch_exterior_workspace_bytes(const tuch_contact_model* model, int B);
int tuch_exterior_flags(const tuch_contact_model* model, const float* verts, int B, int apply_segments,
                        float thresh, float* w, uint8_t* exterior, float* seg_w, uint8_t* seg_exterior,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Winding numbers of arbitrary points against the model's mesh posed by `verts`, loss.py:295-297
 * (HD points offset along the face normals).  points [B,Q,3] (padded); counts [B] device ints or
 * NULL: meaningful points per body; padded entries give w = 0, exterior = 1. */
size_t tuch_winding_points_workspace_bytes(const tuch_contact_model* model, int B, int Q);
int tuch_winding_points(const tuch_contact_model* model, const float* verts, const float* points,
                        const int32_t* counts, int B, int Q, float thresh, float* w, uint8_t* exterior,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Closest point on the posed surface (csrc/closest_point.hip).  For every real query p of points [B,Q,3]: d2 [B,Q] is
 * the squared distance to the nearest point c of the model's mesh posed by verts [B,V,3], face [B,Q] a face that
 * attains it, bary [B,Q,3] the weights with c = sum_k bary[k] * verts[faces[face][k]], each in [0,1], their sum 1
 * within rounding.  A face without area (coincident or collinear corners) counts as its edges: the nearest point of the
 * segment or the point, finite outputs.
 *   The rule: the squared distance of a (query, triangle) pair is one fixed instruction sequence, independent of group,
 * lane, batch and visiting order; the winner is the smallest d2, among faces whose d2 have the same bits the smallest
 * face index (a packed minimum of d2 bits << 32 | face).  So a query gives the same bits alone or in any batch, for any
 * order of the queries, eager or replayed.  Groups of faces (the cluster tree's leaves, or runs of 64 faces for a mesh
 * without a tree) are skipped by their posed boxes only when no face of them can produce a smaller or equal key: the
 * float32 box bound carries a margin of 64 * 2^-24 times the squared distance to the box's farthest corner (derivation
 * in the source file), and the outputs equal an unpruned sweep bit for bit.
 *   counts [B] device ints or NULL: real queries per body (clamped to [0, Q]); entries at or beyond counts[b] get
 * d2 = +inf, face = -1, bary = 0.  Every index read from the tables is clamped before it is used as an address.  A
 * body with NaN or Inf vertices or points changes no other body's bits and yields face indices in [-1, F).  B = 0 or
 * Q = 0: nothing is done.  No allocation, no synchronisation, capturable; the workspace
 * (tuch_closest_point_workspace_bytes: boxes [B,G,8] and the posed corners in group order [B,F,9]; with oriented != 0,
 * which a call with normals needs, also the cones [B,G,8]) is guarded under option canary.
 *   hint [B,Q] device ints or NULL.  hint[b,q] names a face that is probably the answer -- in a fitting loop the face the
 * previous iteration returned.  It is only a bound: d2, face and bary equal those of the call with hint = NULL bit for bit
 * for EVERY content of hint (the right face, a wrong one, -1, F, INT32_MAX, INT32_MIN, any mix within a wavefront).  A
 * hint in [0, F) -- checked before it is used as an address -- makes the query start from that face's exact distance and
 * group instead of from the walk over every box of the body; any other value, or a hinted face whose distance is not
 * finite (NaN vertices), takes the unhinted path.  hint may alias the face output: a lane reads its own hint before it
 * writes its face, so a loop can keep one [B,Q] tensor that is both.
 *   normals (optional) [B,Q,3] or NULL (float32, any length, in the frame of verts): the normal-compatible search, with
 * max_angle_cos = c, the float32 cosine of an angle in (0, 90] degrees (the caller computes the cosine in double and
 * rounds it once); c outside [0, 1) or not finite is an argument error.  With normals = NULL max_angle_cos is ignored
 * whatever it holds.  A query is (p, n); a face is a candidate only if it is ADMISSIBLE for n.
 *   The admissibility rule, one fixed float32 sequence, every product, sum and difference rounded on its own (nothing
 * fused), for a face with posed corners a, b, c (the bits of verts) and c2 = c * c formed once in float32:
 *     e1 = b - a, e2 = c - a                       (one subtraction per component)
 *     m = e1 x e2                                  (each component as (x * y) - (z * w))
 *     mm = (mx*mx + my*my) + mz*mz,  nn = (nx*nx + ny*ny) + nz*nz,  s = (mx*nx + my*ny) + mz*nz
 *     admissible  <=>  s > 0  and  s * s >= c2 * (mm * nn).
 * A face without area (mm = 0, s = 0) is never admissible for a constrained query; neither is one with NaN corners
 * (every comparison is false).  A query whose nn is 0 or not finite (a missing normal: a zero row, NaN, Inf, overflow)
 * is UNCONSTRAINED: every face is admissible and its three outputs have the bits of the call without normals.
 *   The winner is the smallest packed key d2 bits << 32 | face over the admissible faces, d2 from the unchanged
 * distance sequence; a query without an admissible face gets d2 = +inf, face = -1, bary = 0.  A query gives the same
 * bits alone or in any batch, for any order of the queries, eager or replayed, for any grouping of the faces and for
 * every content of hint: the outputs equal an unpruned sweep over all faces under this rule, bit for bit (groups are
 * skipped by their boxes as before, and by per-group normal cones whose margins are conservative: derivation in the
 * source file).  A hinted query starts from its hint only if the face is in [0, F), admissible for it and at a finite
 * d2; any other hint takes the unhinted path.  counts, NaN bodies, B = 0 or Q = 0 and the aliasing of hint with face
 * as above.  tuch_closest_point_bwd applies to the outputs unchanged (face = -1 contributes nothing); normals are
 * constants and get no gradient. */
size_t tuch_closest_point_workspace_bytes(const tuch_contact_model* model, int B, int Q, int oriented);
int tuch_closest_point(const tuch_contact_model* model, const float* verts /* [B,V,3] */,
                       const float* points /* [B,Q,3] */, const float* normals /* [B,Q,3] or NULL */, float max_angle_cos,
                       const int32_t* counts /* [B] or NULL */, const int32_t* hint /* [B,Q] or NULL */, int B, int Q,
                       float* d2 /* [B,Q] */, int32_t* face /* [B,Q] */, float* bary /* [B,Q,3] */, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The face groups the search walks, as host copies (any may be NULL): *num_groups = G, group_off_host [G+1],
 * face_list_host [F] (the faces of group g are face_list[group_off[g] .. group_off[g+1])), face_group_host [F] (the
 * group of every face: the inverse of face_list, where a hinted query starts). */
int tuch_contact_model_face_groups(const tuch_contact_model* model, int* num_groups, int32_t* group_off_host,
                                   int32_t* face_list_host, int32_t* face_group_host);
/* Its adjoint in the envelope form (the weights held fixed: exact wherever the closest feature is locally constant):
 * grad_points [B,Q,3] = 2 g (p - c) is WRITTEN (0 for padded entries and face = -1, which contribute nothing), and
 * -2 g bary[k] (p - c) is added to the rows of the winning face's three corners -- with grad_verts_fixed_zeroed
 * (deterministic mode, as tuch_contact_terms_bwd_fixed) as 64-bit fixed-point integers, grad_verts [B,V,3] then being
 * written from the sums if given; without it as float atomics into a grad_verts the caller has zeroed.  face and bary
 * are tuch_closest_point's outputs; face indices outside [0, F) are skipped. */
int tuch_closest_point_bwd(const tuch_contact_model* model, const float* verts, const float* points,
                           const int32_t* face, const float* bary, const float* grad_d2 /* [B,Q] */, int B, int Q,
                           float* grad_points /* [B,Q,3] written, or NULL */,
                           void* grad_verts_fixed_zeroed /* B*V*3 zeroed 64-bit words, or NULL */,
                           float* grad_verts /* [B,V,3], or NULL */, void* stream);

/* Point-to-surface data term of a fit to unregistered points (csrc/scan_fit.hip).  The queries are points[b,q] -
 * transl[b] (one float32 subtraction per component) against the model's mesh posed by verts[b]: d2, face, bary are
 * those of tuch_closest_point on these queries, bit for bit (counts, hint and its aliasing with face as there).
 *   per_body[b] = sum_{q < counts[b]} w_q rho(d2_q) / sum_{q < counts[b]} w_q,   total[0] = sum_b per_body[b],
 * with weights [B,Q] or NULL (all ones) and rho = 0: d2;  1: sqrt(d2), derivative 0 at d2 = 0;  2: sigma^2 d2 /
 * (sigma^2 + d2) (sigma > 0; ignored otherwise).  A point of weight 0 is not computed from and may be non-finite; a
 * body whose weights sum to 0 or with counts[b] = 0 has per_body = 0 and zero gradient rows.
 *   The gradients of total for a unit upstream gradient, the weights of the nearest point held fixed, with g_q = w_q
 * rho'(d2_q) / sum w and r = (p - t) - c: grad_points [B,Q,3] = 2 g r (or NULL), the rows of the winning face's corners
 * in grad_verts [B,V,3] get -2 g bary_k r, grad_transl [B,3] = -sum_q 2 g r.  grad_verts is zeroed by the call and
 * summed with float atomics, or, under tuch_set_deterministic(1), as 64-bit fixed-point integers in the workspace
 * (the same bits on every call); per_body, its normaliser, total and grad_transl are fixed-order sums in both modes.
 * ticket: one int, zero before the first call and left zero by every call.  No allocation, no synchronisation,
 * capturable; the workspace (tuch_scan_fit_workspace_bytes, with oriented != 0 for a call with normals) is guarded
 * under option canary.
 *   normals (optional) [B,Q,3] or NULL, and max_angle_cos, as in tuch_closest_point: the term over the normal-compatible
 * search.  The queries are points - transl as above; normals are not translated and get no gradient.  d2, face, bary
 * are those of tuch_closest_point with these normals on these queries, bit for bit.  A real point without an
 * admissible face (face = -1) contributes 0 to the loss and to every gradient and KEEPS its weight in the normaliser:
 * an unmatched point adds nothing and the denominator does not move. */
size_t tuch_scan_fit_workspace_bytes(const tuch_contact_model* model, int B, int Q, int oriented);
int tuch_scan_fit_terms(const tuch_contact_model* model, const float* verts /* [B,V,3] */,
                        const float* transl /* [B,3] */, const float* points /* [B,Q,3] */,
                        const float* normals /* [B,Q,3] or NULL */, float max_angle_cos,
                        const int32_t* counts /* [B] or NULL */, const float* weights /* [B,Q] or NULL */,
                        const int32_t* hint /* [B,Q] or NULL */, int B, int Q, int rho, float sigma,
                        float* d2 /* [B,Q] */, int32_t* face /* [B,Q] */, float* bary /* [B,Q,3] */, int* ticket,
                        float* per_body /* [B] */, float* total /* [1] */, float* grad_verts /* [B,V,3] */,
                        float* grad_transl /* [B,3] */, float* grad_points /* [B,Q,3] or NULL */, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Nearest point of a static point cloud; the model -> scan term of a two-sided fit (csrc/point_cloud.hip).  No model
 * is involved: a cloud has no mesh.
 *   The rule.  The cloud of body b is the set of VALID points of points [B,Q,3]: index < counts[b] (counts [B] or NULL,
 * clamped to [0, Q]), weight != 0 where weights [B,Q] are given, all three coordinates finite; any other point is never
 * a neighbour and never computed from (it may be NaN).  The query is q = x + shift[b], one float32 add per component
 * (shift NULL: the bits of x).  THE squared distance of a (query, point) pair is d = q - s per component and
 * d2 = (dx dx + dy dy) + dz dz, every product and sum rounded to float32 on its own (no fused multiply-add).  The
 * winner is the smallest packed key d2 bits << 32 | index, index being the point's position in the caller's [Q] order:
 * the smallest d2, among equal bits the smallest index; only a finite d2 can win, and with max_distance tau > 0 only
 * d2 <= (float)tau * (float)tau, compared in float32 (max_distance <= 0: no limit).  A query without winner -- empty
 * cloud, non-finite query, every valid point beyond tau, an entry at or beyond query_counts[b] -- gets index = -1,
 * d2 = +inf.  A query's outputs have the same bits alone or in any batch, for any order of the queries, for any order
 * in which the build filed the points, for any resolution, eager or replayed, and for EVERY content of hint.  A body
 * with NaN / Inf queries or points changes no other body's bits; every index read from a table is clamped before it
 * addresses anything.  There is no gradient with respect to the points of the cloud: they are data.
 *   tuch_point_cloud_build files the valid points into a uniform grid per body -- isotropic cells, the longest extent of
 * the valid points' box cut into `resolution` (1 .. 256) cells, the header (origin, cell edge, dims) written on the
 * device -- in the workspace (tuch_point_cloud_workspace_bytes: 0 for B, Q or resolution <= 0).  Five kernel launches,
 * no host round trip, no allocation, no synchronisation, capturable.  The query reads points / counts / weights again
 * only to check a hint: pass the arrays the cloud was built from.
 *   hint [B,N] device ints or NULL: hint[b,n] in [0, Q) that names a valid point -- checked before anything is
 * addressed -- whose d2 is finite and within tau gives the lane's starting bound and enters as an ordinary key; any other
 * value takes the unhinted path.  hint may alias index: a lane reads its own entry before it writes it.
 *   Cells and 4^3-cell blocks are skipped only when no point filed in them can produce a key smaller than or equal to
 * the lane's bound; the bound's margin (2^-20, relative, in units of cells) is derived in the source file.
 *   Option canary (tuch_point_cloud_set_canary, process-wide, returns the old value; set it before sizing and building):
 * guard words behind every region of the workspace and of the term's scratch; words found changed are counted in the
 * workspace's first word (zero it once), read -- and reset -- with tuch_point_cloud_canary_hits, which synchronises. */
size_t tuch_point_cloud_workspace_bytes(int B, int Q, int resolution);
int tuch_point_cloud_build(const float* points /* [B,Q,3] */, const int32_t* counts /* [B] or NULL */,
                           const float* weights /* [B,Q] or NULL */, int B, int Q, int resolution, void* workspace,
                           size_t workspace_bytes, void* stream);
/* normals (optional): the oriented query, the rule above over the ADMISSIBLE valid points.  normals [B,Q,3] belong to the
 * points, in the caller's order; query_normals [B,N,3] to the queries (neither is translated by shift).  The two go
 * together: both NULL is the plain query, which ignores max_angle_cos, cones and cones_bytes whatever they hold; one
 * without the other is an argument error.  With c = max_angle_cos in [0, 1) (anything else is an argument error),
 * c2 = c c formed once, for a query normal u and a point normal n, every operation rounded to float32 on its own:
 *   uu = (ux ux + uy uy) + uz uz,  nn = (nx nx + ny ny) + nz nz,  s = (ux nx + uy ny) + uz nz,
 *   admissible  <=>  s > 0  and  s s >= c2 (uu nn).
 * A pair is unconstrained -- admissible -- when uu or nn is 0 or not finite: a missing normal, the zero rows of
 * tuch_point_cloud_normals among them.  Valid points, q = x + shift, the squared distance, the packed key, max_distance,
 * query_counts and the no-winner outputs (-1 / +inf) are the plain query's; the winner is the smallest key over
 * the admissible valid points; a hint seeds the search only if it names a valid, admissible point within the limit.
 * The outputs equal a float32 brute-force sweep under this rule bit for bit: for any batch, order of queries or points,
 * resolution and hint content, eager or replayed, with cones or with cones NULL.
 *   cones: per-block normal cones that let a lane pass by a block of the grid none of whose points is admissible for
 * its normal (they may only skip, never decide; csrc/point_cloud.hip has the derivation).  A caller-provided buffer of
 * tuch_point_cloud_cones_bytes(B, resolution) bytes, filled by tuch_point_cloud_build_cones AFTER tuch_point_cloud_build
 * from the same normals (one launch, capturable) and stale after the next build; NULL: no block is skipped. */
size_t tuch_point_cloud_cones_bytes(int B, int resolution);
int tuch_point_cloud_build_cones(const void* workspace, size_t workspace_bytes, const float* normals /* [B,Q,3] */, int B,
                                 int Q, int resolution, void* cones, size_t cones_bytes, void* stream);
int tuch_point_cloud_nearest(const void* workspace, size_t workspace_bytes, const float* points /* [B,Q,3] */,
                             const int32_t* counts /* [B] or NULL */, const float* weights /* [B,Q] or NULL */,
                             const float* normals /* [B,Q,3] or NULL */, const float* queries /* [B,N,3] */,
                             const float* query_normals /* [B,N,3] or NULL */, const float* shift /* [B,3] or NULL */,
                             const int32_t* query_counts /* [B] or NULL */, const int32_t* hint /* [B,N] or NULL */,
                             float max_distance, float max_angle_cos, const void* cones /* or NULL */, size_t cones_bytes,
                             int B, int Q, int N, float* d2 /* [B,N] */, int32_t* index /* [B,N] */, void* stream);
/* k nearest points, and PCA normals over them.  The rule above, verbatim -- the valid points, q = x + shift[b], THE
 * squared distance, the packed key d2 bits << 32 | index, max_distance, query_counts -- for the k (1 .. 32; anything
 * else is an argument error) smallest keys of a query, in ascending order: index [B,N,k], d2 [B,N,k].  With fewer than
 * k admissible points (finite d2, within tau) the tail is -1 / +inf; a non-finite query, an empty cloud or an entry at
 * or beyond query_counts[b] gives all -1 / +inf.  A point that coincides with the query is an ordinary neighbour with
 * d2 = 0: querying a cloud with its own points returns each point itself first, or the smallest index among its
 * duplicates.  The outputs equal a sorted float32 brute-force sweep bit for bit, alone or in a batch, for any order of
 * queries or points, any resolution, eager or replayed.  One launch, no workspace beyond the cloud's; capturable.
 *   Neighbourhood statistics: one fixed float32 sequence, every product, sum and difference rounded on its own.  With
 * the n <= k neighbours found, in key order, s_j read from `points` (pass the array the cloud was built from):
 *   d_j = s_j - q per component;  m = (...((d_1 + d_2) + d_3)... + d_n) / (float)n;  e_j = d_j - m;
 *   C_ab = ((0 + e_1,a e_1,b) + e_2,a e_2,b) + ... for ab = xx, xy, xz, yy, yz, zz  (cov [B,N,6] or NULL, in that order).
 * C has the same bits whatever the grid, the batch or the order of the points; centring on the query keeps the sums
 * free of the cloud's distance from the origin.
 *   normals [B,N,3]: the unit eigenvector of C's smallest eigenvalue lambda0 <= lambda1 <= lambda2, by cyclic Jacobi in
 * float32 with a fixed number of sweeps.  With T = trace C + n |m|^2 = sum_j |d_j|^2 and E = (n + 256) 2^-24 T (derived
 * in the source file: it bounds the error of C and of the solver against the float64 scatter matrix of the same
 * neighbours; T = trace C for a query at the centroid and T <= (n + 1) trace C for a query that is one of its own
 * neighbours), the sine of the normal's angle error is at most 2 E / (lambda1 - lambda0).  The row is ZERO when n < 3
 * or 2 E >= lambda1 - lambda0 --
 * collinear, coincident or isotropic neighbours, where the bound says nothing; also when T is not finite or below
 * 1e-30, or the solver's residual exceeds 2^-24 T -- which is what tuch_closest_point with normals treats as unconstrained.
 *   variation [B,N] = lambda0 / (lambda0 + lambda1 + lambda2), within 2 E / trace C + 2^-23 of the float64 value; 0 where
 * the normal is zero.  count [B,N] = n.
 *   Sign: first canonical -- the component of the largest magnitude is positive, the first among equals --; then with a
 * viewpoint c (layout 1: [B,3], layout 2: [B,N,3]; the sensor's position in the frame of the queries q) t = c - q,
 * s = (n_x t_x + n_y t_y) + n_z t_z, and the normal is negated when s < 0, kept when s >= 0 or s is not finite.  A
 * query's normal has the same bits alone or in any batch, order or resolution.  weights decide validity only; the PCA
 * is unweighted.  No gradients: the cloud is data. */
int tuch_point_cloud_knn(const void* workspace, size_t workspace_bytes, const float* points /* [B,Q,3] */,
                         const int32_t* counts /* [B] or NULL */, const float* weights /* [B,Q] or NULL */,
                         const float* queries /* [B,N,3] */, const float* shift /* [B,3] or NULL */,
                         const int32_t* query_counts /* [B] or NULL */, float max_distance, int B, int Q, int N, int k,
                         float* d2 /* [B,N,k] */, int32_t* index /* [B,N,k] */, void* stream);
int tuch_point_cloud_normals(const void* workspace, size_t workspace_bytes, const float* points, const int32_t* counts,
                             const float* weights, const float* queries, const float* shift, const int32_t* query_counts,
                             float max_distance, int B, int Q, int N, int k, const float* viewpoint,
                             int viewpoint_layout /* 0 none, 1 [B,3], 2 [B,N,3] */, float* normals /* [B,N,3] */,
                             float* variation /* [B,N] */, int32_t* count /* [B,N] */, float* cov /* [B,N,6] or NULL */,
                             void* stream);
/* The term: the query for q = verts[b,v] + transl[b] (d2, index [B,V] as tuch_point_cloud_nearest gives them; a vertex
 * of weight 0 is not computed from and gets -1 / +inf), vertex weights w NULL (ones; layout 0), [V] (layout 1) or [B,V]
 * (layout 2), rho / sigma as tuch_scan_fit_terms, and
 *   per_body[b] = scale sum_v w_v rho(d2_v) / sum_v w_v,   total[0] = sum_b per_body[b].
 * A vertex without winner contributes rho(tau^2) when max_distance is given and the body's cloud is not empty, 0
 * otherwise, and has a zero gradient row.  A body whose cloud is empty or whose weights sum to 0 has per_body = 0 and
 * zero gradients.  For a unit upstream gradient, the nearest point held fixed: grad_verts[b,v] = 2 g_v (q - s) with
 * g_v = scale w_v rho'(d2_v) / sum w (every row written, by the lane that owns it: no atomics), grad_transl[b] = sum_v
 * grad_verts[b,v].  per_body, its normaliser, total and grad_transl are fixed-order sums: the same bits in either mode
 * of tuch_set_deterministic, on every call, and for a body alone or in a batch.  ticket as for tuch_scan_fit_terms;
 * scratch: tuch_point_cloud_fit_scratch_bytes(B, V) bytes.  One launch; capturable.
 *   normals (optional) [B,Q,3] or NULL: the term with the oriented query.  The lane that owns vertex v forms the vertex's
 * normal itself, from the UNTRANSLATED verts, by tuch_vertex_normals' sequence (faces [F,3], vf_off [V+1], vf_ids [3F]
 * as there, all required, with F > 0 and 3F < 2^31; normalize = 0), so d2 / index have the bits of
 * tuch_point_cloud_nearest called with these normals and tuch_vertex_normals' raw rows as query_normals, and the term
 * stays one launch.  The term, a vertex without winner, the fixed-order sums and the gradients are as above; normals
 * only decide the match and get no gradient.  max_angle_cos and cones as for tuch_point_cloud_nearest.  With normals =
 * NULL the mesh, the cones and max_angle_cos are ignored whatever they hold. */
size_t tuch_point_cloud_fit_scratch_bytes(int B, int V);
int tuch_point_cloud_fit_terms(const void* workspace, size_t workspace_bytes, const float* points, const int32_t* counts,
                               const float* weights, const float* normals /* [B,Q,3] or NULL */, float max_angle_cos,
                               const int32_t* faces, const int32_t* vf_off, const int32_t* vf_ids, int F,
                               const void* cones /* or NULL */, size_t cones_bytes, const float* verts /* [B,V,3] */,
                               const float* transl /* [B,3] */, const int32_t* hint /* [B,V] or NULL */, float max_distance,
                               int B, int Q, int V, const float* vertex_weights, int vertex_weight_layout, int rho,
                               float sigma, float scale, float* d2 /* [B,V] */, int32_t* index /* [B,V] */, int* ticket,
                               float* per_body /* [B] */, float* total /* [1] */, float* grad_verts /* [B,V,3] */,
                               float* grad_transl /* [B,3] */, void* scratch, size_t scratch_bytes, void* stream);
/* Posed vertex normals (csrc/vertex_normals.hip).  vf_off [V+1], vf_ids [3F]: the vertex -> faces lists of
 * tuch_render_mesh (vertex v is a corner of the faces vf_ids[vf_off[v] .. vf_off[v+1]), ascending).  One fixed float32
 * sequence, nothing fused: for vertex v, over its faces in that order, m = (b - a) x (c - a) exactly as
 * tuch_closest_point with normals forms it, u_v = ((0 + m_1) + m_2) + ... per component: the area-weighted normal,
 * unnormalised.  normalize != 0: divided by sqrt(uu), uu = (ux ux + uy uy) + uz uz; a zero row where uu is 0 or not
 * finite.  out [B,V,3], every row written by the lane that owns it: no atomics, the same bits for a vertex alone or in
 * any batch, eager or replayed; table entries are clamped before they address anything; a body that holds NaN changes
 * no other body's bits.  No gradients.  One launch; capturable. */
int tuch_vertex_normals(const float* verts /* [B,V,3] */, const int32_t* faces /* [F,3] */, const int32_t* vf_off,
                        const int32_t* vf_ids, int B, int V, int F, int normalize, float* out, void* stream);
/* Host copies of the per-body headers the build wrote: origin_host [B,3], cell_host [B], dims_host [B,3].  Synchronises;
 * for tests and tools (a test can put points exactly on cell walls). */
int tuch_point_cloud_grid(const void* workspace, int B, int resolution, float* origin_host, float* cell_host,
                          int32_t* dims_host);
int tuch_point_cloud_set_canary(int on);
int tuch_point_cloud_canary_hits(void* workspace, int* hits_host, int reset);

/* region-pair minima: TUCH.contact_from_verts, train_module.py:69-91 (select NULL, unmasked)
 * and the region-to-region term, losses.py:107-117 (select = gt_contact & has_discrete_contact,
 * geodesically masked).  out_min [B,P] (0 where not selected), out_ij [B,P,2] arg-min vertices. */
int tuch_region_pair_min(const tuch_contact_model* model, const float* verts, int B, const uint8_t* select,
                         int use_geomask, float* out_min, int32_t* out_ij, void* stream);
int tuch_region_pair_min_bwd(const tuch_contact_model* model, const float* verts, int B, const int32_t* ij,
                             const float* grad_out, float* grad_verts, void* stream);

/* Self-contact detection (csrc/self_contact.hip): TUCH.get_verts_in_contact, train_module.py:93-110, and the contact
 * signature whose per-body minimum eval.py:135-136 reads from a file.  A pair (i, j) QUALIFIES when its mask bit is set
 * and |v_i - v_j|^2 < euclthres^2 (direct differences, the same bits as tuch_v2v_min_masked / tuch_region_pair_min;
 * euclthres <= 0: nothing qualifies; no special case for i == j: the mask decides).  geomask_bits: tuch_pack_geomask's
 * layout, from it or from tuch_contact_model_mask_bits; the bit of (i, j) is bit j % 64 of word [j / 64][i], i.e.
 * geomask[i][j] of the packed byte matrix -- the reference's `cmask[i][j]` and the orientation tuch_region_pair_min uses
 * for (first region, second region); tuch_v2v_min_masked's minimum for vertex i runs over geomask[j][i]: the same thing
 * for a symmetric mask only.
 * Per vertex i: in_contact = some j qualifies; min_d2 = the minimum over the qualifying j (+inf when none); partner =
 * the smallest j attaining it (-1 when none).  cnc_d2 [B] = minimum over all qualifying pairs of the body (+inf: no
 * contact).  With a region table -- vreg_off [V+1] / vreg: the CSR lists vertex -> region ids in [0, R), R <= 128;
 * regions may overlap or be empty, a vertex may belong to none -- sig_d2 [B,R,R]: sig_d2[b][r1][r2] = minimum over the
 * qualifying pairs with r1 in regions(i) and r2 in regions(j), +inf when none.  vreg_off = NULL: no signature (vreg, R,
 * sig_d2 ignored).  Two launches on `stream` (preset of sig_d2 / cnc_d2, then the search), no workspace, no
 * synchronisation; all minima are order-free: bit-identical from run to run and in any batch.  B = 0: no-op. */
int tuch_self_contact(const float* verts /* [B,V,3] */, const uint64_t* geomask_bits, int B, int V, float euclthres,
                      const int32_t* vreg_off /* [V+1] or NULL */, const int32_t* vreg /* region ids */, int R,
                      uint8_t* in_contact /* [B,V] */, int32_t* partner /* [B,V] */, float* min_d2 /* [B,V] */,
                      float* sig_d2 /* [B,R,R] or NULL */, float* cnc_d2 /* [B] */, void* stream);

/* ---- mesh renderer (csrc/render.hip): what tuch/utils/renderer.py asks of pyrender, on the compute units --------
 * tuch_render_mesh: B bodies x n_views (1..32) views -> face [B,n_views,H,W] (triangle id, -1 = empty), depth (the same
 * shape; camera-space z in metres at the pixel centre, 0 = empty: the reference's `rend_depth > 0`) and image
 * [B,n_views,H,W,3] in [0,1].
 * Camera: utils/geometry.perspective_projection.  p = view_rot[w] v + cam_t[b] lands at (focal p.x / p.z + cx,
 * focal p.y / p.z + cy); the pixel in row r, column c has its centre at (c + 0.5, r + 0.5).
 * Coverage is exact and watertight: the projections are snapped to 1/256 px, the edge functions are 64-bit integers, a
 * centre on an edge belongs to the triangle when the centre moved by (+eps, +eps^2) is strictly inside (top-left rule):
 * exactly one of the triangles that share an edge or a vertex, whatever the face order or winding.  No back-face
 * culling.  A triangle is dropped whole when a corner has p.z <= 1e-3 m, a coordinate that is not finite (or a
 * projection beyond +-2^21 px), an index outside [0,V), or when its snapped area is zero; triangles partly outside the
 * image are clipped to it by their bounding box.
 * Visibility: one 64-bit key per pixel (float bits of z, face id) merged with an atomic minimum -- the nearest surface,
 * at equal depth the smaller face id; z is interpolated perspective-correctly (1 / z linear in screen space) with the
 * barycentrics of the UNSNAPPED float32 projections, clamped to the triangle -- only coverage is decided on the snapped
 * grid.  Order-free: outputs are bit-identical from run to run and for a body alone or inside any batch.
 * Shading: area-weighted vertex normals (gathered through vf_off [V+1] / vf_ids, the vertex -> faces CSR lists, in list
 * order) and the vertex colours, interpolated perspective-correctly; rgb = albedo / 255 * min(1, 0.3 + 0.7 max(0, -n_z))
 * with n in the camera frame: the reference's ambient term and its lights along the viewing direction.  pyrender's
 * physically based look is NOT emulated.  colors [B,V,3] u8 or NULL (230,230,230: renderer.py:185); empty pixels take
 * background [B,H,W,3] in the views whose bit is set in background_views (bit w = view w) and 1.0 elsewhere or when
 * background is NULL.
 * One memset and three launches on `stream`, no synchronisation, capturable.  B = 0: no-op. */
size_t tuch_render_workspace_bytes(int B, int n_views, int V, int F, int H, int W);
int tuch_render_mesh(const float* verts /* [B,V,3] */, const int32_t* faces /* [F,3] */, const int32_t* vf_off /* [V+1] */,
                     const int32_t* vf_ids, int B, int V, int F, const float* cam_t /* [B,3] */,
                     const float* view_rot /* [n_views,3,3] */, int n_views, float focal, float cx, float cy, int H, int W,
                     const uint8_t* colors /* [B,V,3] or NULL */, const float* background /* [B,H,W,3] or NULL */,
                     unsigned int background_views, int32_t* face, float* depth, float* image, void* workspace,
                     size_t workspace_bytes, void* stream);
/* The reference's contact colouring (renderer.py:199-224) for a batch: colors [B,V,3] u8.  meshcols of a body =
 * (v - min_axis) * 255 / max_axis(v - min_axis) in float32, in this order, truncated.  Untouched vertices keep 230.
 * Pair form (pair_off [B+1] != NULL; c1, c2 [n_pairs]: body b owns the pairs pair_off[b] .. pair_off[b+1]): both
 * vertices of pair k get (meshcols[c1[k]] + meshcols[c2[k]]) >> 1; pairs in list order, the last write wins.
 * Region form (contact [B,P] 0/1 != NULL; pairs [P,2] region ids; region_first [R]: the first LISTED vertex of each
 * region, -1 for an empty one; vreg_off / vreg: tuch_self_contact's vertex -> regions table): every vertex of both
 * regions of every active pair gets meshcols[region_first[first region]]; pairs in increasing order, the last wins; a
 * pair whose first region is empty is skipped.  Entries outside their range are ignored.  Three launches, order-free. */
size_t tuch_contact_vertex_colors_workspace_bytes(int B, int V, int R);
int tuch_contact_vertex_colors(const float* verts /* [B,V,3] */, int B, int V, const int32_t* pair_off, const int32_t* c1,
                               const int32_t* c2, int n_pairs, const uint8_t* contact, const int32_t* pairs, int P,
                               const int32_t* region_first, const int32_t* vreg_off, const int32_t* vreg, int R,
                               uint8_t* colors, void* workspace, size_t workspace_bytes, void* stream);

/* ---- SMPL forward / backward: tuch/models/smpl.py:34-56 over smplx 0.1.13 lbs() -------------
 * Model arrays are HOST pointers in the layouts smplx registers them: v_template [V,3],
 * shapedirs [V,3,10], posedirs [207,3V], J_regressor [24,V], lbs_weights [V,24], parents [24],
 * extra_vertex_ids [21] (smplx VertexJointSelector), J_regressor_extra [9,V] and joint_map [49]
 * (models/smpl.py:39-42). */
typedef struct tuch_smpl_model tuch_smpl_model;

int tuch_smpl_model_create(tuch_smpl_model** out, int V, const float* v_template, const float* shapedirs,
                           const float* posedirs, const float* J_regressor, const float* lbs_weights,
                           const int32_t* parents, const int32_t* extra_vertex_ids,
                           const float* J_regressor_extra, const int32_t* joint_map);
void tuch_smpl_model_destroy(tuch_smpl_model* model);
int tuch_smpl_model_info(const tuch_smpl_model* model, int* V);

/* SMPL.forward(betas, body_pose, global_orient, pose2rot) with the pose as its caller holds it (tuch/models/smpl.py:44-47):
 * betas [B,10]; global_orient [B,3] and body_pose [B,69] axis-angle (pose2rot != 0) or [B,1,3,3] and [B,23,3,3] rotation
 * matrices, row strides in floats -> vertices [B,V,3], joints [B,49,3].  One concatenated pose [B,72] (w = 3) or
 * [B,24,3,3] (w = 9): global_orient = pose, body_pose = pose + w, both strides 24 w.
 * The forward workspace keeps the intermediates tuch_smpl_backward_split needs. */
size_t tuch_smpl_forward_workspace_bytes(const tuch_smpl_model* model, int B);
int tuch_smpl_forward_split(const tuch_smpl_model* model, const float* betas, const float* global_orient,
                            int global_orient_stride, const float* body_pose, int body_pose_stride, int pose2rot, int B,
                            float* verts, float* joints, void* workspace, size_t workspace_bytes, void* stream);
/* Adjoint: g_verts [B,V,3] / g_joints [B,49,3] (either may be NULL) -> g_betas [B,10] and the pose gradient as the two
 * tensors of the forward call (same shapes, row strides in floats).
 * g_body_pose_add (same shape as g_body_pose, row stride in floats; or NULL): a gradient the caller already holds for
 * body_pose, g_body_pose = this call's gradient + that one.  In SMPLify-DC body_pose feeds the body model and the pose
 * prior (tuch/smplify/losses.py:63): autograd would add the two gradients in a separate launch.
 * g_verts_fixed (here and in tuch_smpl_backward_split_adam; or NULL): [B,V,3] 64-bit fixed-point sums (2^-36, the
 * accumulators tuch_smplify_stage2_fused leaves in deterministic mode) ADDED to g_verts where the skinning adjoint reads
 * it -- the stage-2 tail's vertex gradient without a conversion launch on the step's serial tail. */
size_t tuch_smpl_backward_workspace_bytes(const tuch_smpl_model* model, int B);
int tuch_smpl_backward_split(const tuch_smpl_model* model, const float* global_orient, int global_orient_stride,
                             const float* body_pose, int body_pose_stride, int pose2rot, int B,
                             const void* fwd_workspace, const float* g_verts, const float* g_joints, float* g_betas,
                             float* g_global_orient, int g_global_orient_stride, float* g_body_pose,
                             int g_body_pose_stride, const float* g_body_pose_add, int g_body_pose_add_stride,
                             void* workspace, size_t workspace_bytes, void* stream, const void* g_verts_fixed);
/* tuch_smpl_backward_split (axis-angle poses) + torch.optim.Adam's update (tuch_adam_step's arithmetic) of the two pose
 * tensors themselves, applied by the last backward kernel to the rows whose gradient it has just written: for a fit whose
 * optimiser holds exactly [global_orient, body_pose] and whose whole gradient arrives through this call (SMPLify-DC stage 2,
 * tuch/smplify/smplifydc.py:149-183: the body model + the pose prior via g_body_pose_add) -- the optimiser's own launch at
 * the end of every iteration is gone.  param_*: the tensors the optimiser updates (normally the memory global_orient /
 * body_pose point to), exp_avg* contiguous [B,3] / [B,69], step: the optimiser's device counter (advanced by one),
 * ticket: one zeroed int the call leaves zero.  The gradients are still written to g_*. */
int tuch_smpl_backward_split_adam(const tuch_smpl_model* model, const float* global_orient, int global_orient_stride,
                                  const float* body_pose, int body_pose_stride, int B, const void* fwd_workspace,
                                  const float* g_verts, const float* g_joints, float* g_betas, float* g_global_orient,
                                  int g_global_orient_stride, float* g_body_pose, int g_body_pose_stride,
                                  const float* g_body_pose_add, int g_body_pose_add_stride,
                                  float* param_global_orient, int param_global_orient_stride, float* param_body_pose,
                                  int param_body_pose_stride, float* exp_avg_global_orient, float* exp_avg_sq_global_orient,
                                  float* exp_avg_body_pose, float* exp_avg_sq_body_pose, float* step, int* ticket,
                                  float lr, float beta1, float beta2, float eps,
                                  void* workspace, size_t workspace_bytes, void* stream, const void* g_verts_fixed);

/* ---- caller-side glue of the training step ----------------------------------------
 * tuch_estimate_translation: tuch/utils/geometry.py:114-205 (estimate_translation + estimate_translation_np):
 * camera translation [B,3] that best projects the model joints onto the 2D keypoints (weighted least squares,
 * weights sqrt(conf)); joints3d [B,J,3], keypoints2d [B,J,3] = (u, v, conf), J = 49; has_anno[b] selects the
 * ground-truth joints [25,J) else the OpenPose joints [0,25); samples whose confidences sum to 0 get zeros.
 * float64 inside, like the reference's numpy.
 * tuch_rotmat_to_angle_axis: torchgeometry 0.1.2 rotation_matrix_to_angle_axis as called at
 * tuch/train/train_module.py:208-212 and demo_smplify_dc.py:128-132; rotmat [N,3,row_stride] with
 * row_stride 3 or 4 (the callers append a homogeneous column); NaN entries propagate and
 * are zeroed by the callers (train_module.py:212). */
int tuch_estimate_translation(const float* joints3d, const float* keypoints2d, const uint8_t* has_anno, int B, int J,
                              float focal_length, float img_size, float* trans, void* stream);
int tuch_rotmat_to_angle_axis(const float* rotmat, int N, int row_stride, float* angle_axis, void* stream);

/* ---- pose evaluation (csrc/pose_eval.hip) -----------------------------------------------------------
 * tuch_procrustes: tuch/utils/pose_utils.py:28-92 (compute_similarity_transform, its _batch loop and
 * reconstruction_error; eval.py:194 calls it once per batch on host copies).  S1, S2 [B,N,D] or, with coords_first,
 * [B,D,N] (the reference reads a per-body matrix whose first axis is 2 or 3 as coordinates x points,
 * pose_utils.py:35-39); D = 2 or 3; float (is_double = 0) or double (1).  S1_hat (optional, same layout and type) =
 * scale R S1 + t with R = V Z U^T from the SVD of K = X1 X2^T; err [B] = reconstruction_error(S1, S2, None): the
 * root of the sum over the LAST axis of the given layout, averaged over the other.  float64 inside; all points of S1
 * equal -> NaN, as in the reference.
 * tuch_pose_metrics: eval.py:158-195 and tuch/train/trainer.py:229-255 for one batch in one launch.
 * pred_vertices [B,V,3]; exactly one of gt_vertices [B,V,3] (regressed like pred, pelvis subtracted) or gt_joints
 * [B,J,3] (the mpi-inf-3dhp branch, eval.py:168-170: used as given); J_regressor [R,V] (R <= 24, every entry used);
 * joint_map [J] (J <= 64; H36M_TO_J14 / _J17) into the R joints; the pelvis (row pelvis_index of the regressed
 * joints) is taken before the map.  Per body: mpjpe [B], pa_mpjpe [B] (tuch_procrustes's error on the mapped
 * joints), v2v [B] (optional; mean vertex distance, gt_vertices only) and joints [B,R,3] (optional; the regressed
 * pred joints before the pelvis, eval.py:184).  Deterministic: no atomics; a body's outputs do not depend on the
 * batch it is in.  A joint_map entry outside [0,R) gives NaN for that body (the binding checks before the launch). */
int tuch_procrustes(const void* S1, const void* S2, int B, int N, int D, int coords_first, int is_double, void* S1_hat,
                    void* err, void* stream);
int tuch_pose_metrics(const float* pred_vertices, const float* gt_vertices, const float* gt_joints,
                      const float* J_regressor, const int32_t* joint_map, int B, int V, int R, int J, int pelvis_index,
                      float* mpjpe, float* pa_mpjpe, float* v2v, float* joints, void* stream);

/* ---- the regressor's input: batched crops and augmentation (csrc/image_crop.hip) ---------------------
 * tuch_crop_batch: tuch/utils/imutils.py:67-106 (crop) and tuch/datasets/base_dataset.py:192-205 (rgb_processing) for B
 * samples in one launch: out [B,channels,R,R] float32 (normalised) and, optionally, raw [B,channels,R,R] in [0,1].
 *
 * Per sample (one tuch_crop_record, built on the host in float64: tuch_amd/ops.py crop_records): a source image, HWC,
 * 1 or 3 channels, uint8 (type 0) or float32 (type 1), `height` x `width` texels, rows `stride` BYTES apart, its first
 * texel `offset` bytes into `buffer`; centre, scale, rot (degrees), flip and the per-channel pixel noise pn.
 *
 * THE RESAMPLING RULE.
 * Box: the reference's integer box, ul = transform([1,1], invert=1) - 1, br = transform([R+1,R+1], invert=1) - 1, both
 * truncated toward zero (imutils.py:73-77), bw = br.x - ul.x, bh = br.y - ul.y (they can differ by one); the pad
 * p = int(|br - ul| / 2 - bh / 2) when rot != 0, else 0 (imutils.py:80-83).  The padded box P has its origin at
 * (ox, oy) = ul - p and the size (pw, ph) = (bw + 2p, bh + 2p).
 * Map: a pixel spans [k, k+1).  A point (xo, yo) of the output, in [0,R)^2, goes to the box, (xo bw / R, yo bh / R), is
 * shifted by p, rotated by +rot about the centre (pw / 2, ph / 2) of P with [[cos, -sin], [sin, cos]] in (x right, y
 * down), and 0.5 is subtracted: texel-index coordinates inside P; adding (ox, oy) gives image texels.  This is the
 * inverse map skimage's rotate and resize compose.  flip mirrors the output: xo -> R - xo.
 * Samples: K = clamp(ceil(max(bw, bh) / R), 1, 16); output pixel (i, j) is the equal-weight mean of the K x K samples at
 * (j + (2u+1) / 2K, i + (2v+1) / 2K), rows v outermost, each a bilinear fetch.  K = 1 is plain bilinear (what the
 * reference does when enlarging); K > 1 stands in for the Gaussian pre-filter skimage applies when shrinking -- a
 * stated deviation.
 * Exact positions: with the integer grid coordinates (gx, gy) = (2K j + 2u + 1, 2K i + 2v + 1), gx -> 2KR - gx under flip,
 *     X = (ax[0] gx + ax[1] gy + ax[2]) >> 16,   Y = (ay[0] gx + ay[1] gy + ay[2]) >> 16      (64-bit, arithmetic shift)
 * are the position in units of 2^-16 px: the coefficients carry 32 fractional bits, round-to-nearest is folded into the
 * constant term, and X deviates from the float64 map by less than 2^-12 px anywhere on the grid (R <= 1024).  The texel is
 * X >> 16, the weight (X & 65535) / 65536: no float decides which texel is read.
 * Fetch: the texel index and its +1 neighbour are clamped into [0, pw-1] x [0, ph-1] (the edge of P is replicated; the
 * reference reflects there), then moved by (ox, oy); a texel outside the image reads 0.  Nothing outside
 * [offset, offset + (height-1) stride + row bytes) is addressed; a record for which that range leaves
 * [0, buffer_bytes), or whose fields are out of range, yields zeros (the binding refuses it on the host before).
 * Value, float32 with every operation spelled out: top = fma(t01, wx, t00 (1-wx)), bottom likewise, sample =
 * fma(bottom, wy, top (1-wy)), summed in sample order, divided by K^2; v = clamp(mean pn_c, 0, 255)
 * (base_dataset.py:200-202); raw = v / 255; out = (raw - mean_c) / std_c.  A float32 source is treated the same way.  A
 * 1-channel source fills every output channel; a 3-channel source needs channels = 3.
 * A box that misses the image gives an all-zero crop (raw = 0), where the reference raises -- a stated deviation.
 *
 * mean / std: `channels` host floats, read during the call.  One launch on `stream`, no allocation, no synchronisation:
 * capturable.  B = 0 is a no-op.  A sample's output does not depend on the batch it is in. */
typedef struct tuch_crop_record {
    int64_t offset, stride;          /* bytes */
    int64_t ax[3], ay[3];            /* the integer affine above */
    int32_t height, width, channels, type;
    int32_t pw, ph, ox, oy;          /* P: size and origin in image texels */
    int32_t K, flip;
    float pn[3];
    int32_t reserved;                /* 120 bytes */
} tuch_crop_record;
int tuch_crop_batch(const void* buffer, size_t buffer_bytes, const tuch_crop_record* records, int B, int res, int channels,
                    const float* mean, const float* std, float* out, float* raw, void* stream);

/* ---- the HD-mesh branch of RegressorLoss.contact_loss, tuch/train/loss.py:274-301, as one device pipeline ----
 * (csrc/hd_contact.hip).  tuch_hd_model holds the HD vertex regressor (loss.py:81-83) as its three non-zeros per
 * row -- hd_idx / hd_w [N,3] -- and faces_vert_is_sampled_from (loss.py:85-87) -- hd_face [N]; all host arrays, copied.
 * It refers to the contact model (faces, geodesic mask, cluster tree), which must outlive it.  Point order is the
 * library's business (the loss is a sum over the points): tuch_hd_model_info reports it (order_host[k] = caller's
 * index of the k-th point). */
typedef struct tuch_hd_model tuch_hd_model;
/* A regressor with up to K (1..8) non-zeros per row: hd_idx / hd_w [N,K], rows with fewer non-zeros padded with weight 0
 * (any valid vertex id); K = 3 is the plain barycentric sampling.  The reference multiplies the DENSE matrix
 * (loss.py:285): a regressor file that is not a plain barycentric sampling (<= 3 non-zeros) still loads. */
int tuch_hd_model_create(tuch_hd_model** out, const tuch_contact_model* contact_model, int N, int K,
                         const int32_t* hd_idx, const float* hd_w, const int32_t* hd_face);
void tuch_hd_model_destroy(tuch_hd_model* model);
int tuch_hd_model_info(const tuch_hd_model* model, int* N, int32_t* order_host);
/* One call = loss.py:274-315 for the whole batch: exterior [B,V] u8, min_d2 [B,V], partner [B,V] int32 are the
 * vertex-level results for the same verts [B,V,3] (tuch_exterior_flags with the segment filter, tuch_v2v_min_model);
 * valid [B] u8 or NULL.  terms [B,2] = (sum over interior HD points of tanh^2(d/0.04), sum over exterior ones of
 * 0.005 tanh^2(d/0.005)); bodies with valid == 0 or without a selected point give (0, 0).  thresh = 0.99.
 * `saved` (tuch_hd_contact_saved_bytes, caller-owned, opaque) carries the selection to tuch_hd_contact_bwd, which
 * OVERWRITES grad_verts [B,V,3] with d(sum_b grad_terms[b,:] . terms[b,:]) / d verts.  All buffers are sized for the
 * worst case (every HD point selected); the actual counts never leave the device: no synchronisation, no allocation. */
size_t tuch_hd_contact_saved_bytes(const tuch_hd_model* model, int B);
size_t tuch_hd_contact_workspace_bytes(const tuch_hd_model* model, int B);
int tuch_hd_contact_fwd(const tuch_hd_model* model, const float* verts, const uint8_t* exterior, const float* min_d2,
                        const int32_t* partner, const uint8_t* valid, int B, float euclthres, float thresh, float* terms,
                        void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
int tuch_hd_contact_bwd(const tuch_hd_model* model, const void* saved, const float* grad_terms, int B,
                        float* grad_verts, void* workspace, size_t workspace_bytes, void* stream);
/* inspection (tests; synchronous copies): counts_host [B]; selected_host [B,N] = caller-order index of the point in
 * every slot, -1 beyond the count (or NULL) */
int tuch_hd_contact_selection(const tuch_hd_model* model, const void* saved, int B, int32_t* counts_host,
                              int32_t* selected_host);
/* per slot (order of tuch_hd_contact_selection): caller-order index of the partner the search found (-1 beyond the
 * count) and the exterior flag of the point; both [B,N] */
int tuch_hd_contact_details(const tuch_hd_model* model, const void* saved, int B, int32_t* partner_host, uint8_t* ext_host);

/* HD points of tuch/train/loss.py:285 (hd = Vert_Regressor[selected] @ verts, a dense [N_hd,6890] matrix with three
 * non-zeros per row): point n belongs to body body_of_point[n] and is HD point hd_of_point[n];
 * points[n] = sum_k hd_w[h][k] * verts[body][hd_idx[h][k]].  verts [B,V,3], hd_idx / hd_w [N_hd,3], points [N,3].
 * The adjoint ADDS into grad_verts [B,V,3] (float atomics; zero it first). */
int tuch_hd_points_fwd(const float* verts, const int32_t* body_of_point, const int32_t* hd_of_point,
                       const int32_t* hd_idx, const float* hd_w, int V, int N, float* points, void* stream);
int tuch_hd_points_bwd(const float* grad_points, const int32_t* body_of_point, const int32_t* hd_of_point,
                       const int32_t* hd_idx, const float* hd_w, int V, int N, float* grad_verts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TUCH_AMD_H */
