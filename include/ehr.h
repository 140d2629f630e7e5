/*
 * ehr.h -- C ABI of libehr_hip.so, the MI355X (gfx950) silhouette-rasterizer behind EasyHeC's mask-render hot path.
 *
 * Drop-in boundary: the reference reaches its renderer only through four nvdiffrast.torch entry points
 *     dr.RasterizeCudaContext()                      /root/reference/easyhec/structures/nvdiffrast_renderer.py:23
 *     dr.rasterize(glctx, pos, tri, resolution)      .../nvdiffrast_renderer.py:39  (and :64)
 *     dr.interpolate(attr, rast, tri)                .../nvdiffrast_renderer.py:42  (and :67)
 *     dr.antialias(color, rast, pos, tri)            .../nvdiffrast_renderer.py:43  (and :68)
 * nvdiffrast's own torch plugin binds those to C++ functions taking torch tensors; this header is what a
 * ctypes / pybind stub binds instead (easyhec_amd/_lib.py).  Plain pointers and sizes only.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer on the ctx's / current HIP device unless the name ends in _host;
 *   - all floats are fp32, all indices int32, tensors are dense row-major ("contiguous");
 *   - every call enqueues on `stream` (a hipStream_t; NULL = the null stream) and never blocks, EXCEPT where a
 *     function's comment says "synchronises";
 *   - return value: 0 = ok, negative = error; ehr_last_error() returns the message for the calling thread;
 *   - image rows follow nvdiffrast (row 0 = bottom) for the three drop-in ops; the fused op takes and returns
 *     images in the reference's final convention (row 0 = top, i.e. after nvdiffrast_renderer.py:47's flip).
 */
#ifndef EHR_H
#define EHR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EHR_OK 0
#define EHR_ERR_INVALID (-1)   /* bad argument */
#define EHR_ERR_HIP (-2)       /* a HIP runtime call failed */
#define EHR_ERR_OVERFLOW (-3)  /* internal work buffer overflow (reported, never silent) */
#define EHR_ERR_RETRY (-4)     /* the step was reported as NaN for a reason the library has already fixed: run it again */

typedef struct ehr_ctx ehr_ctx;

/* library / device --------------------------------------------------------------------------------------------- */
int ehr_version(void);                 /* ABI version, currently 8 (8: ehr_antialias_fwd_zg; 7: ehr_comm_p2p_*; 6: tile flags -- ehr_tile_flags_bytes, a tile_flags argument on ehr_rasterize_fwd / _grad, ehr_interpolate_fwd / _grad, ehr_antialias_fwd; 2: ehr_fused_plan takes the scene arrays; 3: ehr_fused_bind_ref, ehr_comm_*, history_row; 4: ehr_ctx_scratch_bytes; 5: EHR_ERR_RETRY from ehr_fused_status, ehr_antialias_fwd needs no zeroed work buffer and out != color, ehr_interpolate_da_*, ehr_rasterize_grad_db) */
const char* ehr_last_error(void);      /* message of the last failing call on this thread ("" if none) */
int ehr_device_count(void);            /* number of visible HIP devices (0 if none) */
const char* ehr_device_arch(int dev);  /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */

/* replaces dr.RasterizeCudaContext() -- nvdiffrast_renderer.py:23.  Owns binning scratch, grown on demand. */
int ehr_ctx_create(int device, ehr_ctx** out);
int ehr_ctx_destroy(ehr_ctx* ctx);
/* Device memory the context holds at the moment (its scratch buffers; they grow on demand and are released with it). */
size_t ehr_ctx_scratch_bytes(ehr_ctx* ctx);

/* replaces dr.rasterize -- nvdiffrast_renderer.py:39.
 * instance mode (ranges_host == NULL): pos [B,V,4], every image draws all T triangles.
 * range mode: pos [V,4], image b draws triangles ranges_host[2b] .. +ranges_host[2b+1] (HOST int32 [B,2]).
 * rast [B,H,W,4] = (u, v, z/w, triangle_id+1); rast_db [B,H,W,4] = (du/dx, du/dy, dv/dx, dv/dy) or NULL.
 * Two forms, same bits.  Small launches (B x T <= 131072: one link's mesh in one image, the reference's call) are
 * depth-tested straight into a key image in global memory and shaded by a second kernel: no queues, never a host wait.
 * Larger ones go through per-tile queues (count, allocate, fill, one workgroup per tile); that form synchronises only
 * while it is sizing its queue storage (first calls of a shape): in steady state the size of a frame reaches the host
 * asynchronously and is looked at by the next call, and a frame that outgrows the storage is still rendered exactly (the
 * tiles whose queues did not fit find their triangles themselves; slower, never incomplete) before the storage grows.
 * Neither form enqueues a fill: the context's counters / key image are left clean by the call's last kernel. */
/* tile_flags (optional, NULL = not wanted): ehr_tile_flags_bytes(B, H, W) bytes, one per (image, 32 x 8 pixel tile, row-major,
 * ceil(W / 32) per row), set to non-zero iff some pixel of the tile holds a triangle (the queued form sets them all).  The
 * ops below that take `tile_flags` leave `rast` unread where the flag is zero: a robot link covers a few per cent of a
 * frame, and the reference's schedule is five full-image passes per (view, link).  Passing NULL there is always valid. */
size_t ehr_tile_flags_bytes(int B, int H, int W);
int ehr_rasterize_fwd(ehr_ctx* ctx, const float* pos, const int32_t* tri, const int32_t* ranges_host, int B, int V,
                      int T, int H, int W, float* rast, float* rast_db, unsigned char* tile_flags, void* stream);

/* backward of dr.rasterize w.r.t. pos through (u,v); dy = grad of rast [B,H,W,4] (z/w and id carry no gradient).
 * grad_pos (pos's shape) is ACCUMULATED into: the caller zero-fills it. */
int ehr_rasterize_grad(const float* pos, const int32_t* tri, const float* rast, const float* dy, int range_mode, int B,
                       int V, int T, int H, int W, float* grad_pos, const unsigned char* tile_flags, void* stream);
/* ... and w.r.t. pos through rast_db: ddb = grad of rast_db [B,H,W,4]; grad_pos is ACCUMULATED into.  (EasyHeC discards
 * rast_db, nvdiffrast_renderer.py:39; this completes the op.) */
int ehr_rasterize_grad_db(const float* pos, const int32_t* tri, const float* rast, const float* ddb, int range_mode, int B,
                          int V, int T, int H, int W, float* grad_pos, void* stream);

/* replaces dr.interpolate -- nvdiffrast_renderer.py:42.  attr [Ba,V,A] with Ba == B or 1; out [B,H,W,A]. */
int ehr_interpolate_fwd(const float* attr, const float* rast, const int32_t* tri, int B, int Ba, int V, int T, int A,
                        int H, int W, float* out, const unsigned char* tile_flags, void* stream);
/* grad_attr [Ba,V,A] is ACCUMULATED into (caller zero-fills) and may be NULL when the attributes need no gradient
 * (EasyHeC interpolates constant colours); grad_rast [B,H,W,4] is overwritten. */
int ehr_interpolate_grad(const float* attr, const float* rast, const int32_t* tri, const float* dy, int B, int Ba, int V,
                         int T, int A, int H, int W, float* grad_attr, float* grad_rast, const unsigned char* tile_flags,
                         void* stream);

/* dr.interpolate's second output, the attribute pixel differentials (interpolate(attr, rast, tri, rast_db, diff_attrs);
 * EasyHeC does not ask for them -- nvdiffrast_renderer.py:42 passes neither -- they complete the op's signature).
 * rast_db [B,H,W,4] from ehr_rasterize_fwd; diff_idx [D] int32 DEVICE attribute indices, NULL = all (then D == A);
 * out_da [B,H,W,2D] = (d attr_j / dX, d attr_j / dY) for j = diff_idx[i] at channels 2i, 2i+1; 0 where no triangle.
 * grad: grad_attr [Ba,V,A] is ACCUMULATED into (may be NULL), grad_rast_db [B,H,W,4] overwritten (may be NULL); rast
 * itself receives no gradient from the differentials. */
int ehr_interpolate_da_fwd(const float* attr, const float* rast, const float* rast_db, const int32_t* tri,
                           const int32_t* diff_idx, int B, int Ba, int V, int T, int A, int D, int H, int W, float* out_da,
                           void* stream);
int ehr_interpolate_da_grad(const float* attr, const float* rast, const float* rast_db, const int32_t* tri,
                            const int32_t* diff_idx, const float* dy_da, int B, int Ba, int V, int T, int A, int D, int H,
                            int W, float* grad_attr, float* grad_rast_db, void* stream);

/* replaces dr.antialias_construct_topology_hash(tri).  Writes opp [T,3] int32: for triangle t and edge k
 * (k=0: v1-v2, k=1: v2-v0, k=2: v0-v1) the third vertex of the other triangle sharing that edge, or -1.
 * scratch: ehr_topology_scratch_bytes(T) bytes of device memory. */
size_t ehr_topology_scratch_bytes(int T);
int ehr_antialias_topology(const int32_t* tri, int T, int32_t* opp, void* scratch, size_t scratch_bytes, void* stream);

/* replaces dr.antialias -- nvdiffrast_renderer.py:43.  color/out [B,H,W,C]; pos [B,V,4] or [V,4] (range_mode).
 * work: ehr_antialias_work_bytes(B,H,W) bytes, filled by fwd and consumed by grad (nvdiffrast's work buffer); it needs
 * no initialisation.  out must not alias color (every pixel reads its neighbours' colours).  The forward result is
 * deterministic: every pixel adds the blends that land on it in the order of a serial sweep over pixel pairs. */
size_t ehr_antialias_work_bytes(int B, int H, int W);
int ehr_antialias_fwd(const float* color, const float* rast, const float* pos, const int32_t* tri, const int32_t* opp,
                      int range_mode, int B, int V, int T, int H, int W, int C, float* out, void* work,
                      const unsigned char* tile_flags, void* stream);
/* The same forward pass, which also clears grad_pos_zero (pos's shape; may be NULL) on its way: the buffer a later
 * ehr_antialias_grad accumulates into then needs no fill of its own -- one launch less per (view, link) image of the
 * reference's schedule (ABI 8).  A caller that runs the backward pass twice zero-fills the buffer itself the second time. */
int ehr_antialias_fwd_zg(const float* color, const float* rast, const float* pos, const int32_t* tri, const int32_t* opp,
                         int range_mode, int B, int V, int T, int H, int W, int C, float* out, void* work,
                         const unsigned char* tile_flags, float* grad_pos_zero, void* stream);
/* grad_color [B,H,W,C] is overwritten (may be NULL: not wanted); grad_pos (pos's shape) is ACCUMULATED into (caller zero-fills). */
int ehr_antialias_grad(const float* color, const float* rast, const float* pos, const int32_t* tri, const float* dy,
                       const void* work, int range_mode, int B, int V, int T, int H, int W, int C, float* grad_color,
                       float* grad_pos, void* stream);

/* Fused hot path: what RBSolver.forward + loss.backward() compute per optimisation step
 * (/root/reference/easyhec/modeling/models/rb_solve/rb_solver.py:60-72 through nvdiffrast_renderer.py:33-47),
 * for B views x L links in one pass:
 *     si[b,l]  = flip_y(antialias(interpolate(1, rasterize(MVP[b,l] * verts_l, tri_l))))
 *     mask[b]  = min(sum_l si[b,l], 1)                 -> mask [B,H,W] (may be NULL)
 *     loss[b]  = sum_pixels (mask[b] - ref[b])^2       -> loss [B]
 *     grad_mvp[b,l] = d loss[b] / d MVP[b,l]           -> grad_mvp [B,L,16] (may be NULL: forward only)
 * Scene = all links concatenated: verts [V,3]; tris [T,3] with GLOBAL vertex indices, sorted by link;
 * tri_link [T] / vert_link [V] int32 link of each triangle / vertex; opp [T,3] from ehr_antialias_topology on the
 * concatenated mesh (links share no vertices, so the per-link topology is preserved).
 * ehr_fused_plan prepares the context for one scene and shape (it synchronises and reads the scene back once): it
 * sizes the scratch for (B,L,V,T,H,W) and builds the static acceleration index of the scene's triangles (clusters of 64
 * spatially close triangles per link, padded index tables), so it takes the scene arrays -- the SAME device arrays that
 * are later passed to ehr_render_mask_loss / ehr_solver_step (they are checked by address; call it again when the
 * scene, the shape or the arrays change -- also when only the CONTENTS of verts / tris change: the index holds a copy
 * of every triangle's corners).  Limits, checked here: L <= 32, W <= 32736, H <= 32760, <= 262144 triangles per link.
 * Any number of views: a call's views go through the launch chain in chunks (one chunk up to 512 / L views; fewer per
 * chunk when the chunk's scratch -- clip-space vertices, raster records, 2 KB per (view, link, tile) job slot: 0.06 GB per
 * 1280x720 view of an 8-link robot -- would exceed 24 GB, EHR_VB_SCRATCH_MB), all inside the one call.  The hot calls never synchronise or allocate, so they can be
 * captured in a hipGraph; a new plan invalidates a captured graph.  `slack` <= 0 (default): one job slot per (view, link,
 * tile), nothing can overflow except the fixed-point accumulators (|sum| > 2^31) and a 16 MB spill pool for tiles with
 * more than 64 blended pairs per link; `slack` > 0 provides only `slack` job slots per view tile (fractions allowed:
 * 0.5 = half as many slots as the view has tiles; less scratch, larger chunks).  An overflow makes loss[] NaN (never a silently wrong image), leaves the optimiser state untouched, and
 * ehr_fused_status() returns EHR_ERR_OVERFLOW after synchronising. */
int ehr_fused_plan(ehr_ctx* ctx, int B, int L, int V, int T, int H, int W, float slack, const float* verts,
                   const int32_t* tris, const int32_t* tri_link, const int32_t* opp);
int ehr_render_mask_loss(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* tri_link,
                         const int32_t* vert_link, const int32_t* opp, const float* mvp, const float* ref, int B,
                         int L, int V, int T, int H, int W, float* mask, float* loss, float* grad_mvp, void* stream);
int ehr_fused_status(ehr_ctx* ctx); /* synchronises the device; 0, EHR_ERR_OVERFLOW or EHR_ERR_RETRY (see ehr_solver_step) */

/* Binds a reference-mask batch ref [B,H,W] (the planned shape) to the plan.  The reference masks of a solve do not
 * change (rb_solver.py:70 compares every step with the same dps['mask']), so the part of the frame loss that comes from
 * image tiles no link touches -- sum(ref^2) over those tiles, 90 % of a 1280x720 frame -- is a constant of the solve.
 * This call stores it once (one pass over ref: per tile the fixed-point value the composite stage would add, per view the
 * total); afterwards ehr_render_mask_loss / ehr_solver_step calls that pass THIS pointer visit only the tiles inside the
 * views' link boxes and correct the cached total by integer differences (with a mask output they also store zeros to
 * every other tile of `mask`, without reading ref there).  The sums are 64-bit fixed point, so loss, gradients and masks
 * are bit-identical to the unbound path; it is an exact algebraic saving, not skipped work.  The caller promises not to
 * modify ref's contents while it is bound: call again after changing them, or with ref == NULL to unbind.
 * ehr_fused_plan unbinds.  Calls with another pointer take the unbound path.  Enqueues on `stream`; not to be called
 * inside a graph capture. */
int ehr_fused_bind_ref(ehr_ctx* ctx, const float* ref, void* stream);
/* The same for a plan whose B = P x Bv views are P hypotheses looking at the SAME Bv images (ehr_solver_step_multi): ref
 * [Bv,H,W] is read P times by this call and never copied; the cached sums (a few KB per view) are stored once per
 * hypothesis, so that view p * Bv + j finds those of image j under its own index.  Bv must divide the planned B;
 * Bv == B is ehr_fused_bind_ref.  A step only takes the bound path when it passes this pointer AND shares it the same way. */
int ehr_fused_bind_ref_shared(ehr_ctx* ctx, const float* ref, int Bv, void* stream);

/* Per-pixel weights of the mask loss, for pixels whose observed mask cannot be trusted (an occluder, motion blur, the
 * frame's edge; 0 = "don't know").  weight [Bv,H,W] float32, row 0 = top like ref.  STICKY state of the plan: until the
 * next call of this function every ehr_render_mask_loss, ehr_solver_step and ehr_solver_step_multi on this context computes
 *     loss[b]          = sum_px  w[b % Bv, px] * (mask[b, px] - ref[b, px])^2
 *     d loss / d mask  = 2 w (mask - ref)   where the links' sum is <= 1, else 0          (the clamp's gate is unchanged)
 * per pixel in float32 as  e = m - r; we = w * e; loss += we * e; g = 2.f * we  -- with w == 1.0f the unweighted
 * expression bit for bit; with w == 0 the pixel adds nothing and its blended pairs are skipped.  The rendered mask does
 * not depend on the weights.  Bv must divide the planned B (view b reads image b % Bv: Bv == B for a solo solve, the Bv of
 * ehr_solver_step_multi for hypotheses that share their images).  weight == NULL unbinds; ehr_fused_plan unbinds.
 * Domain: finite, w >= 0.  Nothing is validated: a NaN, an infinite or a huge weight meets the accumulators' per-addend
 * guard (|addend| >= 1e9) like a bad reference value does, and the step is REPORTED -- NaN loss, optimiser state
 * untouched, ehr_fused_status raised -- never silently wrong.
 * The call UNBINDS a bound reference (its cached sums are sums of w ref^2 and would be stale): bind the weights first,
 * then the reference, which then caches the weighted sums with the composite stage's own expression, so the bound path
 * stays bit-identical to the unbound one.  It also destroys a captured graph (ehr_graph_*), like ehr_fused_bind_ref, and
 * is refused inside a capture.  The caller promises not to modify the weights while they are bound.  Enqueues nothing.
 * ehr_version() is unchanged: the presence of this symbol is the capability check. */
int ehr_fused_bind_weight(ehr_ctx* ctx, const float* weight, int Bv, void* stream);

/* Gauss-Newton information matrix of the fused mask loss for N caller-given tangents dmvp[k] = d MVP / d theta_k
 * ([N,B,L,16] float32; 1 <= N <= 32, anything else is refused).  On the planned context, with the bound weights and a
 * bound reference honoured like ehr_render_mask_loss does.  Per pixel p of view b, with s_p the float32 link sum, m_p the
 * composited mask, e_p = m_p - ref_p, w_p the bound weight (or 1) and gate_p = (s_p <= 1):
 *     J_p[k]  = gate_p * sum_l <d si_l,p / d MVP[b,l], dmvp[k,b,l]>     (the composite stage's blended-pair terms, float32)
 *     info[b] = sum_p w_p J_p J_p^T            [B,N,N] float64, exactly symmetric
 *     grad[b] = sum_p 2 w_p e_p J_p            [B,N]   float64: the loss gradient along the tangents
 *     count[b] = pixels with w_p > 0 and some J_p[k] != 0                [B] int64
 * Per view; sums over views, cameras or hypotheses are the caller's, in float64.  loss [B] and grad_mvp [B,L,16] (both may
 * be NULL) are what ehr_render_mask_loss gives, bit for bit: the call runs that chain and, per chunk of views, one more
 * kernel over the chunk's job slots plus a fixed-order float64 reduction.  No atomics on values: two calls, or two
 * contexts, give identical bits.  A reported call (the chain's overflow, a spill index outside the pool, a slot beyond
 * the plan's, a non-finite sum) leaves info, grad and loss NaN and count -1, and raises ehr_fused_status.  The context's
 * heavy-job hint, bound reference and weights and a solve's optimiser state are as they were afterwards; a natively
 * captured chain stays valid.  Not to be called inside a graph capture (its scratch is sized on the first call).
 * ehr_version() is unchanged: the presence of this symbol is the capability check. */
int ehr_mask_information(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* tri_link,
                         const int32_t* vert_link, const int32_t* opp, const float* mvp, const float* dmvp, int N,
                         const float* ref, int B, int L, int V, int T, int H, int W, double* info, double* grad,
                         long long* count, float* loss, float* grad_mvp, void* stream);

/* Measurement hook (bench.py's roofline leg): when enabled, every ehr_render_mask_loss / ehr_solver_step call records
 * hipEvents around its kernels on the launch stream.  ehr_fused_timing_read synchronises, writes the ACCUMULATED
 * milliseconds per stage since the last read and the number of calls covered, then resets.  Stages of the default
 * (visibility-buffer) chain: ms[0] vertex kernel (pose forward, clip-space vertices, per-triangle raster records, cluster
 * and link boxes), ms[1] job kernel (one wave per (view, link, tile): box culling, LDS rasterizer, depth tests where the
 * silhouette analysis will look, and the resolve stage of the job it has just drawn: silhouette analysis, antialiased
 * values, blended pairs; the dominant kernel -- followed, once a step has needed it, by the general-triangle pass, whose
 * waves likewise resolve what they redraw), ms[4] composite kernel (link sum, clamp, loss, mask, backward; its
 * finisher workgroup runs the finish stage: accumulators -> loss / grad_mvp [-> pose backward -> Adam]).  ms[2] is the
 * place of a resolve launch the chain does not have: always an EMPTY pair of events, it measures what a pair costs on
 * this stack (every other figure includes about as much); ms[3], ms[5], ms[6] are unused (~0).
 * Not for use under graph capture. */
#define EHR_FUSED_STAGES 7
int ehr_fused_timing(ehr_ctx* ctx, int enable);
int ehr_fused_timing_read(ehr_ctx* ctx, float* ms, int* ncalls);

/* The two ends of one optimisation step around the renderer (trainer/rbsolver.py:29-43), each a single tiny kernel so
 * that a whole step is a handful of launches with no host round trip:
 *   ehr_pose_forward : dof[6] -> Tc_c2b = se3_exp_map(dof) (utils/pytorch3d_se3.py:46-130) ->
 *                      mvp[b,l] = proj(K) @ opencv2blender @ Tc_c2b @ link_poses[b,l]   (rb_solver.py:52,63;
 *                      nvdiffrast_renderer.py:33-37).  tc_jac [7,16]: Tc_c2b and d Tc_c2b / d dof_i (forward mode).
 *                      If history != NULL, row step[0] of history [history_rows,6] receives dof (rb_solver.py:50-51).
 *   ehr_pose_backward: grad_mvp [B,L,16] (= d loss_b / d mvp[b,l]) and loss [B] -> red[8] =
 *                      {d(sum_b loss_b)/d dof (6), sum_b loss_b, B}: the 8 floats one all-reduce(sum) exchanges.
 *   ehr_pose_adam    : torch.optim.Adam step (L2 weight decay added to the gradient) on dof with the MEAN-loss
 *                      gradient red[0..5] / red[7]; m, v [6] and step [1] are the optimiser state; loss_out[0] =
 *                      red[6] / red[7]; grad_out [6] optional.  K is the 3x3 row-major intrinsics matrix. */
int ehr_pose_forward(const float* dof, const float* K, const float* link_poses, int B, int L, int H, int W, float n,
                     float f, float* mvp, float* tc_jac, const int32_t* step, float* history, int history_rows,
                     void* stream);
int ehr_pose_backward(const float* grad_mvp, const float* loss, const float* K, const float* link_poses,
                      const float* tc_jac, int B, int L, int H, int W, float n, float f, float* red, void* stream);
int ehr_pose_adam(float* dof, float* m, float* v, int32_t* step, const float* red, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float* loss_out, float* grad_out, void* stream);

/* One whole optimisation step (trainer/rbsolver.py:29-43) as a chain of 3 launches (vertex + raster records; jobs, which
 * resolve themselves; composite + finish.  A fourth -- the general-triangle pass for jobs with a triangle that crosses the
 * near plane or is wider than 512 pixels -- joins the chain once a step has needed it: that step is reported as NaN like an overflow -- loss,
 * gradient NaN, optimiser state untouched --, ehr_fused_status() then returns EHR_ERR_RETRY and switches the pass on for
 * the context's later calls; run the step again, and re-capture the chain if it was captured in a graph.  A robot in
 * front of the camera never has such a triangle; the stateless ehr_render_mask_loss always launches the pass):
 * ehr_pose_forward is merged into the vertex kernel (which also does the per-step housekeeping) and ehr_pose_backward +
 * ehr_pose_adam into the finish stage of the composite kernel.  Same arithmetic and outputs as calling the pieces one by one:
 * mvp [B,L,16], tc_jac [7,16], loss_b [B], grad_mvp [B,L,16], red [8], loss_out [1], grad_out [6] are all written.
 * `step` [1] is Adam's step count (bias correction); `history_row` [1] is the row of history [history_rows,6] that
 * receives this step's pose (rb_solver.py:50-51: the first free row) and is advanced by the call -- two counters,
 * because a solver built on a loaded model starts a fresh optimiser but keeps appending to the history.  history ==
 * NULL records nothing.  A REPORTED step (overflow: NaN loss, pose and optimiser state untouched) has recorded the unchanged
 * pose; the next call of this context notices that neither `step` nor `history_row` has moved since and writes into the
 * SAME row again, so the history holds one row per effective step -- on every rank of a data-parallel job alike (the NaN
 * travels with the exchanged sums), without the caller rewinding anything (ABI 7).
 * defer_adam != 0 stops after `red` so that the caller can exchange it across ranks and then apply Adam: ehr_comm_p2p_step
 * (exchange + Adam in one launch), or ehr_comm_allreduce / any all-reduce followed by ehr_pose_adam.
 * Requires ehr_fused_plan for (B,L,V,T,H,W); never synchronises or allocates. */
int ehr_solver_step(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* tri_link,
                    const int32_t* vert_link, const int32_t* opp, const float* K, const float* link_poses,
                    const float* ref, int B, int L, int V, int T, int H, int W, float near_plane, float far_plane,
                    float* dof, float* adam_m, float* adam_v, int32_t* step, float* history, int history_rows,
                    int32_t* history_row, float lr, float beta1, float beta2, float eps, float weight_decay, float* mvp,
                    float* tc_jac, float* mask, float* loss_b, float* grad_mvp, float* red, float* loss_out,
                    float* grad_out, int defer_adam, void* stream);

/* Multi-start solve: P hypotheses (start poses) of ONE problem of Bv views advance by one optimisation step each, in one
 * launch chain whose length does not depend on P.  Hypothesis p on real view j is virtual view b = p * Bv + j of a
 * P x Bv-view plan (ehr_fused_plan with B = P * Bv; chunked like any other call):
 *     K [9], link_poses [Bv,L,16], ref [Bv,H,W]          passed ONCE, shared: view b reads real view b % Bv, no copies;
 *     dof, adam_m, adam_v [P,6], step [P], history [P,history_rows,6] (may be NULL), history_row [P]   per hypothesis;
 *     mvp, grad_mvp [P*Bv,L,16], loss_b [P*Bv], mask [P*Bv,H,W] (may be NULL)                           per virtual view;
 *     tc_jac [P,7,16], red [P,8], loss_out [P], grad_out [P,6] (may be NULL)                            per hypothesis.
 * The chain is ehr_solver_step's -- vertex kernel (its head reads dof[p]; the first workgroup of every hypothesis's first
 * view writes that hypothesis's tc_jac and history row), jobs, [general-triangle pass], composite -- followed by ONE more
 * small launch with a workgroup per hypothesis that runs the finish stage (accumulators -> loss_b / grad_mvp -> pose
 * backward -> Adam) on that hypothesis's Bv views: 4 launches, 5 with the general-triangle pass.  Within a hypothesis every
 * sum is the expression tree of ehr_solver_step with B = Bv, so hypothesis p's outputs and state equal, bit for bit,
 * those of a solo solve from start p.
 * Failure semantics.  A hypothesis whose own red[p] is not finite is frozen like a reported solo step (dof, moments, step
 * untouched, loss_out[p] = NaN); the others proceed.  The capacity conditions -- job slots, the spill pool, the
 * general-triangle pass switching on, the accumulator range flag -- are STEP-WIDE: the step is reported for every
 * hypothesis (all NaN, all states untouched, every history row reused by the next call) and recovered as for
 * ehr_solver_step (ehr_fused_status; plan again / call again, re-capture a graph).  Known limitation: the accumulator
 * range flag is one word, so one hypothesis whose sums leave +-2^31 reports the step for all; Adam moves a coordinate by
 * at most lr per step, so a hypothesis cannot run away within a solve.
 * Works with ehr_fused_bind_ref_shared, ehr_fused_status, ehr_graph_* and ehr_fused_timing (ms[4] is the composite launch,
 * ms[5] the finish launch) like ehr_solver_step; never synchronises or allocates.  There is no defer_adam: the
 * data-parallel exchange of hypotheses is out of scope.  ehr_version() is unchanged: the presence of this symbol is the
 * capability check. */
int ehr_solver_step_multi(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* tri_link,
                          const int32_t* vert_link, const int32_t* opp, const float* K, const float* link_poses,
                          const float* ref, int P, int Bv, int L, int V, int T, int H, int W, float near_plane,
                          float far_plane, float* dof, float* adam_m, float* adam_v, int32_t* step, float* history,
                          int history_rows, int32_t* history_row, float lr, float beta1, float beta2, float eps,
                          float weight_decay, float* mvp, float* tc_jac, float* mask, float* loss_b, float* grad_mvp,
                          float* red, float* loss_out, float* grad_out, void* stream);

/* The data-parallel exchange (replaces the DDP gradient all-reduce of trainer/base.py:349-352 under the
 * one-process-per-GPU launch of tools/run_easyhec.py:41-50).  Views shard over the ranks; per step every rank runs
 * ehr_solver_step(defer_adam = 1) on its views, the ranks sum the 8-float vector red = [d sum(loss)/d dof (6), sum(loss),
 * n_views] and then run ehr_pose_adam, bit-identically.  The library owns an RCCL communicator per context and issues
 * ncclAllReduce on the stream it is given -- the chain's own stream -- so the step is [solver step, all-reduce, Adam] on ONE
 * stream with no host round trip, and the three calls can be captured together in a hipGraph (ehr_graph_*).
 *   ehr_comm_unique_id : rank 0 obtains the 128-byte ncclUniqueId; the caller ships it to every rank (any transport);
 *   ehr_comm_init      : every rank, with the same id: ncclCommInitRank on the context's device (blocks until all ranks
 *                        have joined); nranks == 1 is legal (a single-GPU communicator);
 *   ehr_comm_allreduce : in-place sum of red[0..count) (device, fp32) over the ranks, enqueued on `stream`;
 *   ehr_comm_destroy   : releases the communicator (ehr_ctx_destroy does it too).
 * RCCL is resolved with dlopen at the first call (the librccl a host process already holds is reused). */
int ehr_comm_unique_id(void* id128_host);
int ehr_comm_init(ehr_ctx* ctx, const void* id128_host, int nranks, int rank);
int ehr_comm_allreduce(ehr_ctx* ctx, float* red, int count, void* stream);
int ehr_comm_destroy(ehr_ctx* ctx);

/* The same exchange WITHOUT a collective library (ABI 7; SURVEY 5 / 8e's one-shot exchange over xGMI peer memory): a step of
 * ~70 us has no room for a 10-30 us ncclAllReduce followed by a launch of its own for Adam.  Every rank owns a mailbox in its
 * device memory; the exchange is one single-workgroup kernel per rank and step that stores the rank's 8 floats and a sequence
 * number into its slot of every peer's mailbox (system-scope stores), waits for its own mailbox to fill, adds the slots up in
 * rank order (bit-identical sums on every rank) and goes on to the Adam update of ehr_pose_adam in the same launch.
 *   ehr_comm_p2p_export : allocates (once) and clears this context's mailbox and returns its 64-byte hipIpcMemHandle; the
 *                         caller ships every rank's handle to every rank (any transport, e.g. an all_gather);
 *   ehr_comm_p2p_open   : handles [nranks][64] in rank order (the own entry is ignored); opens the peers' mailboxes
 *                         (hipIpcOpenMemHandle: ranks on different GPUs of one node, or -- for tests -- on the same GPU);
 *                         nranks <= EHR_P2P_MAX_RANKS.  Every rank must have exported before any rank opens, and opened
 *                         before any rank exchanges (the caller's barrier).
 *   ehr_comm_p2p_step   : red[8] (device) <- sum over the ranks, in place; with dof != NULL the Adam update of ehr_pose_adam
 *                         follows in the same kernel (same arguments).  Every rank must make the same sequence of calls.
 *                         Enqueued on `stream`, capturable.  A peer that never answers is REPORTED after ~half a minute: the sums are NaN
 *                         and the optimiser state stays as it was.
 *   ehr_comm_p2p_close  : closes the peers' mailboxes and frees the own one (ehr_ctx_destroy does it too). */
#define EHR_P2P_MAX_RANKS 64
int ehr_comm_p2p_export(ehr_ctx* ctx, void* handle64_host);
int ehr_comm_p2p_open(ehr_ctx* ctx, const void* handles_host, int nranks, int rank);
int ehr_comm_p2p_step(ehr_ctx* ctx, float* red, float* dof, float* m, float* v, int32_t* step, float lr, float beta1,
                      float beta2, float eps, float weight_decay, float* loss_out, float* grad_out, void* stream);
int ehr_comm_p2p_close(ehr_ctx* ctx);

/* hipGraph capture of launch chains.  ehr_graph_begin opens a capture on a stream the context owns and returns it; every
 * library call made with THAT stream until ehr_graph_end (e.g. one ehr_solver_step, or ehr_solver_step with defer_adam
 * followed by ehr_pose_adam) is recorded instead of executed, including the chain's side-stream fork/join.  All device
 * pointers and scalars of the recorded calls are baked in: the buffers must stay alive and in place; iteration state
 * (dof, Adam moments, step counter, history row) lives on the device, so replays advance the optimisation exactly like
 * eager calls.  ehr_graph_launch enqueues one replay on `stream`.  One graph per context; ehr_graph_begin discards the
 * previous one.  The plan (ehr_fused_plan) must not change between capture and replay. */
int ehr_graph_begin(ehr_ctx* ctx, void** capture_stream);
int ehr_graph_end(ehr_ctx* ctx);
int ehr_graph_launch(ehr_ctx* ctx, void* stream);
int ehr_graph_release(ehr_ctx* ctx);

/* Next-best-view scoring of the space explorer (modeling/models/rb_solve/space_explorer.py:152-165): for each of Q
 * candidate joint configurations, the robot (all links merged into one mesh, utils/render_api.py:70-96) is rendered
 * WITHOUT antialiasing under S camera poses (mask = rast[..., 2] > 0, structures/nvdiffrast_renderer.py:70) and the
 * per-pixel unbiased variance over the S masks is summed over the image (torch.var(masks, dim=0).sum()).  For binary
 * masks that is  sum_px c (S - c) / (S (S - 1))  with c = number of poses covering the pixel, so the kernel returns the
 * exact integer  score[q] = sum_px c (S - c)  and the caller divides.
 *   verts [V,3], tris [T,3] (global vertex ids), vert_link [V] (link of each vertex; NULL = all 0),
 *   mvp [Q,S,L,16] = proj(K) @ opencv2blender @ Tc_c2b[s] @ link_pose[q,l], row-major;
 *   score [Q] int64 (device); count [Q,H,W] uint8 (device, optional; image convention row 0 = top): c per pixel.
 * Two implementations, same integers.  Where the mesh's triangles are grouped by link (vert_link given, every triangle's
 * vertices in one link, links ascending), L <= 32 and S x L <= 512, the call runs on the solver's machinery: the
 * static cluster index of the mesh (built at the first call, rebuilt when the arrays' contents change: a content hash is
 * taken every call), then per chunk of candidates the vertex kernel, the job kernel in a coverage-only form (a triangle
 * all of whose coverable pixels have a depth in (0, 1] needs no depth test at all; the few others are tested per pixel)
 * and a count kernel; one synchronisation at the start (hash) and one at the end.  If a drawn pixel turns out to have a
 * depth <= 0, or a triangle crosses the near plane or spans > 512 pixels -- geometry within two near-plane distances of
 * the camera --, the call is redone by the other implementation: per-triangle tile queues and an exact z-buffer, in
 * passes of about chunk_views rendered views (<= 0: default 512), one synchronisation per pass.
 * EHR_SCORE_PATH=tile / =chain (environment) forces one of them (chain: an error where it cannot decide). */
int ehr_mask_variance(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* vert_link,
                      const float* mvp, int Q, int S, int L, int V, int T, int H, int W, int64_t* score,
                      uint8_t* count, int chunk_views, void* stream);

/* Pose search: mask overlap of Q candidate camera poses with the observed masks of S real views -- the question the local
 * solve cannot answer, "which of these few thousand candidate poses is most worth refining?".  The render rule is exactly
 * ehr_mask_variance's (packed mesh, no antialiasing, a pixel is set iff its nearest fragment has z/w > 0); a pixel of ref
 * is foreground iff ref > 0.5f (NaN is background; dataset masks are 0/1 floats, so any threshold inside (0, 1) agrees).
 *   mvp [Q,S,L,16]: candidate pose q seen in real view s, = proj(K) @ opencv2blender @ Tc_c2b[q] @ link_pose[s,l];
 *   ref [S,H,W] float32 observed masks, row 0 = top (the form ehr_render_mask_loss takes);
 *   overlap [Q,S,2] int64 (device): {inter, area} with area = |render|, inter = |render & ref_s|;
 *   ref_area [S] int64 (device): |ref_s|.
 * From these, |render xor ref| = area + ref_area - 2 inter is the SSE the solver minimises, without antialiasing, and
 * inter / (area + ref_area - inter) the silhouette IoU.  All outputs are exact integers, independent of launch order.
 * Same two implementations, same conditions and same argument limits as ehr_mask_variance.  On the solver's machinery
 * the masks are packed once per call into the bit layout of the job kernel's coverage words (32 bytes per view and
 * 32x8 tile), and per chunk of candidates a count kernel ANDs and popcounts the words: no image reaches memory and no
 * float atomic is used.  If coverage cannot decide a pixel (see above), the WHOLE call is redone by the per-triangle tile
 * implementation on the Q x S single-pose views, in passes of at most chunk_views views (<= 0: default 512), each reduced
 * against ref to the same integers.  EHR_SCORE_PATH=tile / =chain means the same thing.
 * Like ehr_mask_variance the call synchronises (the mesh's content hash at the start, the "coverage could not decide" flag
 * at the end, the queue sizes of every pass of the exact path) and may allocate: it is NOT capturable in a hipGraph.
 * ehr_version() is unchanged: the presence of this symbol is the capability check. */
int ehr_mask_overlap(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* vert_link, const float* mvp,
                     const float* ref, int Q, int S, int L, int V, int T, int H, int W, int64_t* overlap,
                     int64_t* ref_area, int chunk_views, void* stream);

/* Pose search, soft score.  |render xor ref| ranks a candidate that no longer overlaps the observed
 * mask by how SMALL it renders; a cost image built from the distance to the observed mask ranks it by how FAR it is.
 *
 * ehr_mask_distance: exact capped squared Euclidean distance transform of the observed masks.
 *   ref [S,H,W] float32, row 0 = top; a pixel is foreground iff ref > 0.5f (NaN is background): ehr_mask_overlap's rule;
 *   d2 [S,H,W] int32 (device) = min(cap_px^2, min over the foreground (x', y') of (x - x')^2 + (y - y')^2): 0 on the
 *   foreground, cap_px^2 everywhere in a view without foreground;
 *   cap_px in [1, 4096], else EHR_ERR_INVALID with a message.
 * Two passes, every decision in integers (column distances as u16, then per row the minimum of dx^2 + g^2 over the
 * columns within the cap, from an LDS-staged window): exact for every cap_px in the range, no float rounding anywhere.
 * The call only launches on `stream`: no synchronisation, nothing read back.  Its scratch (2 bytes per pixel) comes from
 * the context and only grows: once a call of the same size has been made the call is capturable in a hipGraph.
 *
 * ehr_mask_cost: per (candidate, view) the sums of up to four int32 cost images under the render.
 *   verts .. mvp, Q, S, L, V, T, H, W: as for ehr_mask_overlap (same render rule, same argument limits);
 *   cost [C,S,H,W] int32, row 0 = top, any values; C in [1, 4];
 *   sums [Q,S,C+1] int64 (device): {area, sum_0, .., sum_{C-1}} with area = |render| and
 *   sum_c = sum over the pixels of the render of cost[c,s,pixel].
 * The sums are exact and independent of launch order (64-bit integer atomics only; H W <= 2^30, so they cannot overflow).
 * Same two implementations as ehr_mask_overlap, same chunk_views and EHR_SCORE_PATH.  On the coverage chain the cost
 * images are packed once per call into a tile-major layout in the coverage words' bit order (1 KB per channel, view and
 * 32x8 tile; pixels beyond W or H cost 0), and per chunk of candidates a count kernel fetches the values only under
 * (candidate, view, tile) words that are not zero.  If coverage cannot decide a pixel the WHOLE call is redone by the
 * per-triangle tile implementation on the Q x S single-pose views, in passes of at most chunk_views views (<= 0: 512),
 * each reduced against the cost images to the same integers.  Like ehr_mask_overlap the call synchronises and may
 * allocate: NOT capturable.
 * ehr_version() is unchanged: the presence of these two symbols is the capability check. */
int ehr_mask_distance(ehr_ctx* ctx, const float* ref, int S, int H, int W, int cap_px, int32_t* d2, void* stream);
int ehr_mask_cost(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* vert_link, const float* mvp,
                  const int32_t* cost, int C, int Q, int S, int L, int V, int T, int H, int W, int64_t* sums,
                  int chunk_views, void* stream);

/* Joint-offset calibration: the joint zero errors of the arm are fitted together with the camera pose.  Two small kernels
 * AROUND the launch chain of ehr_solver_step, which itself is unchanged: it reads link_poses from device memory on every call
 * and leaves grad_mvp [B,L,16] and the pose it rendered (tc_jac[0:16]) behind.  A step is
 *     ehr_joint_forward -> ehr_solver_step -> ehr_joint_backward_adam        on one stream.
 * Both calls take device pointers only, never allocate or synchronise, and launch on `stream`: between ehr_graph_begin and
 * ehr_graph_end they are captured together with the chain.
 * The kinematic chain is a flat table in articulation order (UrdfChain.joint_table; N <= 64 links, J <= 32 active joints):
 *   parent [N] int32 (-1 = root; a parent precedes its child), origin [N,16] float64 row-major, kind [N] int32 (0 fixed,
 *   1 revolute / continuous, 2 prismatic), axis [N,3] float64 unit, qidx [N] int32 (active joint that moves the link, or -1),
 *   use [L] int32 (the rendered links), upstream [L] uint32 (bit j: active joint j lies between the root and rendered link l).
 * The caller validates the table (it is device memory here); a malformed one gives NaN outputs, never an access outside the arrays.
 *   ehr_joint_forward : qpos [B,J] float64, offset [J] float32 ->  T_child = T_parent @ origin @ motion(q_j + offset_j), walked
 *                       in float64 and rounded ONCE: link_poses [B,L,16] float32 (at offset == 0 the float32 cast of the host's
 *                       float64 forward kinematics up to the double rounding, i.e. within one float32 unit of max(1, |x|)) and
 *                       joint_frames [B,J,6] float32 = (a, p): the world axis of active joint j in view b and a world point on
 *                       it.  One wave per view, the link frames in LDS; any B.
 *   ehr_joint_backward_adam : with G = (PF @ Tc)^T @ grad_mvp[b,l], PF = proj(K) @ opencv2blender and Tc = tc_jac[0:16] (NOT
 *                       recomputed from dof, which Adam has already moved), and R_l, t_l from link_poses[b,l]:
 *                           d(sum_b loss_b) / d offset_j = sum_{b,l : bit j of upstream[l]} <G, D_blj>
 *                           revolute  D = [ [a]x R_l | a x (t_l - p) ; 0 0 ]      prismatic  D = [ 0 | a ; 0 0 ]
 *                       summed in float64 in a fixed order (bit-reproducible), then ehr_pose_adam's update per element on the
 *                       mean-loss gradient g_j = sum / red[7] with L2 weight decay, where free_joints[j] != 0 only: a joint that
 *                       is not free keeps its offset and moments and reports grad_out[j] = 0.  joint_kind [J] int32 is the kind of
 *                       the link each active joint moves; offset, adam_m, adam_v [J] and step_j [1] are this parameter group's
 *                       own state (its own step counter); grad_out [J] may be NULL.  red [8] is the solver step's: if any of
 *                       red[0..7] is not finite (a REPORTED step: same `< 3.0e38f` test as the pose's Adam) the offsets, the
 *                       moments and step_j stay untouched and the free joints' grad_out is NaN -- the next forward launch then
 *                       writes identical link_poses, so the chain's own recovery (the same history row again, the
 *                       general-triangle pass, a new plan) works unchanged.  A single workgroup.
 * Out of scope: a data-parallel job (the offset gradient would need an exchange of its own) and ehr_solver_step_multi (the
 * hypotheses share ONE link_poses; the multi-start Levenberg-Marquardt solve has ehr_joint_forward_multi, below).  ehr_version() is unchanged: the presence of these symbols is the capability check. */
int ehr_joint_forward(const int32_t* parent, const double* origin, const int32_t* kind, const double* axis,
                      const int32_t* qidx, const int32_t* use, int N, int J, int L, const double* qpos, const float* offset,
                      int B, float* link_poses, float* joint_frames, void* stream);
int ehr_joint_backward_adam(const float* grad_mvp, const float* tc_jac, const float* K, int B, int L, int J, int H, int W,
                            float near_plane, float far_plane, const float* link_poses, const float* joint_frames,
                            const uint32_t* upstream, const int32_t* joint_kind, const float* red, const int32_t* free_joints,
                            float* offset, float* adam_m, float* adam_v, int32_t* step_j, float lr, float beta1, float beta2,
                            float eps, float weight_decay, float* grad_out, void* stream);

/* Camera-rig calibration: C fixed cameras watch ONE arm, and every camera constrains the same joint offsets.  Each camera runs
 * its own  ehr_joint_forward (with the SHARED offset pointer, into its own link_poses / joint_frames) -> ehr_solver_step(
 * defer_adam = 1)  on its own context, views, K and image size; then ONE launch of a single 256-thread workgroup finishes the
 * step for the whole rig.  `cams` is a DEVICE array of C <= 16 structs of device pointers (what camera c's chain left behind,
 * and its pose's Adam group); L and J are the rig's (one robot).  No atomics, no allocation, no synchronisation; capturable.
 *   per camera, in order : S_c[j] = the float64 sum ehr_joint_backward_adam forms for that camera alone (same expressions,
 *                          tiles starting at that camera's pair 0, same order, same combination of the four waves);
 *   the rig              : T[j] = S_0[j] + S_1[j] + ... in float64, n = red_0[7] + red_1[7] + ... in float32 (camera order),
 *                          g_j = (float)T[j] / n: the gradient of the MEAN per-view loss over all views of all cameras.
 *                          With C == 1 every value is ehr_joint_backward_adam's, bit for bit.
 *   all or nothing       : ok = every red_c[0..7] of every camera passes ehr_pose_adam's `< 3.0e38f` test (and every B_c is in
 *                          range: B_c >= 1, B_c * L <= INT_MAX / 16 -- the array is device memory, so this is judged on the
 *                          device, and such a camera is read nowhere).  If ok, camera c's dof / adam_m / adam_v / step get
 *                          ehr_pose_adam's update on its own red_c (pose_lr, pose_wd; loss_out[0] = red_c[6] / red_c[7],
 *                          grad_out [6] optional) bit for bit, and the free joints get ehr_joint_backward_adam's update on g_j
 *                          with the offsets' own counter step_j, offset_lr and offset_wd; a joint that is not free keeps
 *                          everything and reports offset_grad_out[j] = 0.  If not ok, NOTHING moves -- no camera's pose group,
 *                          not the offsets' -- every camera's loss_out (and grad_out) is NaN and the free joints'
 *                          offset_grad_out is NaN: a report is rig-wide, as it is step-wide in ehr_solver_step_multi, and every
 *                          camera's chain re-uses its history row on the next call by its own rule.
 * ehr_version() is unchanged: the presence of this symbol is the capability check. */
typedef struct {            /* one camera of the rig; all pointers are device pointers */
    const float *grad_mvp, *tc_jac, *K, *link_poses, *joint_frames, *red;   /* what that camera's chain left behind */
    float *dof, *adam_m, *adam_v; int32_t *step;  float *loss_out, *grad_out; /* its pose's Adam group */
    int B, H, W;  float near_plane, far_plane;
} ehr_rig_camera;

int ehr_rig_backward_adam(const ehr_rig_camera* cams /* DEVICE array [C] */, int C, int L, int J,
        const uint32_t* upstream, const int32_t* joint_kind, const int32_t* free_joints,
        float* offset, float* adam_m, float* adam_v, int32_t* step_j,
        float pose_lr, float offset_lr, float beta1, float beta2, float eps, float pose_wd, float offset_wd,
        float* offset_grad_out, void* stream);

/* Intrinsics refinement: the focal lengths and the principal point are fitted together with the camera pose.  ONE small kernel
 * AFTER the launch chain of ehr_solver_step, which itself is unchanged: it reads K (nine floats) from device memory on every
 * call and leaves grad_mvp [B,L,16] and the pose it rendered (tc_jac[0:16]) behind.  A step is
 *     ehr_solver_step -> ehr_intrinsics_backward_adam        on one stream
 * (with joint offsets: ehr_joint_forward -> ehr_solver_step -> ehr_joint_backward_adam -> ehr_intrinsics_backward_adam; the
 * joint kernel reads K as rendered, so the launch that rewrites K runs last).  Device pointers only; never allocates or
 * synchronises; launches on `stream`: between ehr_graph_begin and ehr_graph_end it is captured together with the chain.
 *   parameters : K0 [9] float32 = the intrinsics as given (never written), theta [4] float32, dimensionless:
 *                    fu = K0[0] exp(theta0)    fv = K0[4] exp(theta1)    cu = K0[2] + W theta2    cv = K0[5] + H theta3
 *   writing K  : K[0], K[4], K[2], K[5] are evaluated in float64 and rounded once; the other five entries are K0's; an entry
 *                whose theta is exactly 0 is written with K0's bits (selected, not left to exp(0) == 1).
 *   gradient   : A_bl = F @ Tc @ link_poses[b,l] with F = diag(1,-1,-1,1) and Tc = tc_jac[0:16] (NOT recomputed from dof, which
 *                Adam has already moved), Q[r,k] = sum_{b,l} sum_c grad_mvp[b,l][r,c] A_bl[k,c], and for d(sum_b loss_b)/d theta
 *                    s0 = fu (2/W) Q[0,0]    s1 = fv (2/H) Q[1,1]    s2 = -2 Q[0,2]    s3 = 2 Q[1,2]
 *                with fu, fv as rendered (from theta BEFORE this update).  Products and sums are float64 from float32 inputs in
 *                a fixed order, no atomics: thread t of the single 256-thread workgroup adds pairs t, t + 256, ... in order,
 *                each wave combines by a shuffle butterfly, the four waves add in order.  Bit-reproducible.
 *   free, tie  : free4 [4] int32; an element that is not free keeps theta and its moments and reports grad_out == +0.  With
 *                tie_focal != 0 both focal elements take s0 + s1, the derivative with respect to ONE common log-scale: from
 *                equal starts (theta, moments) they stay equal bit for bit.
 *   Adam       : ehr_pose_adam's update per element on g_i = (float)s_i / red[7] with L2 weight decay; theta, adam_m, adam_v
 *                [4] and step_k [1] are this parameter group's own state (its own counter, lr and weight decay); grad_out [4]
 *                may be NULL.  red [8] is the solver step's: if any of red[0..7] fails the pose Adam's `< 3.0e38f` test (a
 *                REPORTED step), or a free element's float32 sum does, nothing of the group moves, K is left as it is and the
 *                free elements' grad_out is NaN -- the chain then renders the same K again and its own recovery (the same
 *                history row again, the general-triangle pass, a new plan) works unchanged.
 * Out of scope: per-camera intrinsics inside ehr_rig_backward_adam, a data-parallel job (the gradient would need an exchange of
 * its own), ehr_solver_step_multi (the hypotheses share ONE K), lens distortion, skew, per-view intrinsics.
 * ehr_version() is unchanged: the presence of this symbol is the capability check. */
int ehr_intrinsics_backward_adam(const float* grad_mvp, const float* tc_jac, const float* link_poses, int B, int L,
                                 int H, int W, const float* red, const float* K0, const int32_t* free4, int tie_focal,
                                 float* theta, float* adam_m, float* adam_v, int32_t* step_k, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, float* K, float* grad_out, void* stream);

/* Levenberg-Marquardt on the information matrix: a damped Gauss-Newton solve of the fused mask loss whose iteration is
 *     [ehr_joint_forward, if joints are free] -> ehr_lm_linearize -> ehr_mask_information -> ehr_lm_update      on one stream,
 * with no host round trip: the state of the solve lives in a device block (below).  Both calls take device pointers only, never
 * allocate or synchronise and launch on `stream`.  Adam's moments, its step counters and the pose history are not touched, and
 * there is no weight decay unless the caller asks for a Gaussian prior (ehr_lm_update_prior, below): this is a refinement beside
 * the Adam solves, not a replacement.
 * The N <= EHR_LM_MAX_PARAMS parameters are ordered as easyhec_amd.information.information_of orders them: dof[0..5], then
 * offset[free_list[0..F)], then the free intrinsics in the order f (tie_focal: theta[0] and theta[1] as one) | fx, fy, then cx, cy;
 * free4_mask has bit i set where theta[i] is free (tie_focal needs bits 0 and 1), and N = 6 + F + Fi.
 *   ehr_lm_linearize : mvp [B,L,16] = ehr_pose_forward's, bit for bit (the same device functions: the solve minimises exactly the
 *                      loss the Adam solve reports), and dmvp [N,B,L,16] = d MVP[b,l] / d parameter k, evaluated in float64 at
 *                      the float32 inputs and rounded once.  With PF = proj(K) @ diag(1,-1,-1,1) and K as rendered:
 *                          pose        PF @ (d Tc / d dof_i) @ link_poses[b,l]        (the exponential map's partials in float64)
 *                          offset j    PF @ Tc @ D_blj, D as for ehr_joint_backward_adam; exactly zero where bit j of
 *                                      upstream[l] is clear.  joint_frames, upstream, joint_kind: ehr_joint_forward's / the table's
 *                          intrinsics  (d proj / d theta_i) @ diag(1,-1,-1,1) @ Tc @ link_poses[b,l]: the derivatives that s0..s3 of
 *                                      ehr_intrinsics_backward_adam imply (2 fu / W, 2 fv / H, -2, 2), fu, fv = K[0], K[4];
 *                                      tie_focal: the sum of the two focal tangents.
 *                      One thread per (k, b, l) matrix.  F == 0: the joint pointers may be NULL.
 *   ehr_lm_update    : one workgroup, float64, fixed order, no atomics.  info [B,N,N], grad [B,N], count [B], loss [B]: the outputs
 *                      of ehr_mask_information at the trial the previous call wrote.  In order:
 *                      1. H = sum_b info[b], g = sum_b grad[b], F = sum_b (double) loss[b], in view order.
 *                      2. Any non-finite sum or a count < 0 (a REPORTED call): the accepted parameters are written back,
 *                         `reported` is incremented, nothing else moves -- the next iteration renders the accepted point again.
 *                      3. The first call accepts unconditionally; later ones iff F < F_acc.  Accept: the parameters (read back
 *                         through the pointers), F, H, g and the pixel count are stored, rho = (F_acc - F) / pred,
 *                         lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2.  Reject: lambda *= nu, nu *= 2, H_acc and g_acc stay
 *                         (the call's inputs are not read again).
 *                      4. (H_acc + lambda D) delta = -g_acc / 2, D = diag H_acc, solved as the scaled system
 *                         (S H_acc S + lambda I) y = -S g_acc / 2, S = D^-1/2, delta = S y, by a Cholesky factorisation.  A
 *                         parameter whose diagonal entry is <= 0 is left out (delta = 0).  A non-positive pivot raises lambda
 *                         like a rejection and factors again, 8 times at the most (`retries`); then done with why = 4.
 *                         pred = delta^T H_acc delta + 2 lambda delta^T D delta  >= 0  (from F(theta + delta) ~ F + g^T delta +
 *                         delta^T H delta with the op's conventions).
 *                      5. The stopping rule: pred <= ftol F_acc (why 1), else lambda >= lambda_max (2), else every |delta_k| is
 *                         zero or below the float32 spacing at the accepted parameter (3).  It sets `done`; the accepted
 *                         parameters are written back, and every later call only does that.  finalize != 0 does it on request.
 *                      6. Otherwise the trial fl32(theta_acc + delta) is written through dof, offset and theta; where intrinsics
 *                         are free, K is rewritten from theta by the "writing K" rule of ehr_intrinsics_backward_adam.
 *                      N < 6 is accepted where nothing but the pose is free: the first N pose coordinates alone.
 *                      log (may be NULL): [log_rows,4] float64; the call that is iteration i < log_rows writes row i =
 *                      {F (NaN: reported), 1 accepted / 0 rejected / -1 reported, lambda after the call, rho (NaN unless accepted)}.
 * The state block: EHR_LM_STATE_DOUBLES float64 (counters and flags are whole numbers, the accepted parameters float32 values,
 * both held exactly).  The caller clears it and sets EHR_LM_LAMBDA (lambda_0) and EHR_LM_NU (2) before the first call.
 * ehr_version() is unchanged: the presence of these symbols is the capability check. */
#define EHR_LM_MAX_PARAMS 32
#define EHR_LM_LAMBDA 0      /* the damping */
#define EHR_LM_NU 1          /* its growth factor on the next rejection */
#define EHR_LM_F 2           /* F_acc: the loss at the accepted point */
#define EHR_LM_PRED 3        /* predicted reduction of the last solve */
#define EHR_LM_RHO 4         /* gain ratio of the last acceptance */
#define EHR_LM_F_TRIAL 5     /* the loss of the last trial that was not reported */
#define EHR_LM_ITERATIONS 6  /* calls that were iterations: accepted + rejected + reported */
#define EHR_LM_ACCEPTED 7
#define EHR_LM_REJECTED 8
#define EHR_LM_REPORTED 9
#define EHR_LM_DONE 10
#define EHR_LM_WHY 11        /* 1 ftol, 2 lambda_max, 3 step below float32's spacing, 4 the factorisation kept failing */
#define EHR_LM_LAST 12       /* the last iteration: 1 accepted, 0 rejected, -1 reported */
#define EHR_LM_COUNT 13      /* sum_b count[b] at the accepted point */
#define EHR_LM_RETRIES 14    /* non-positive pivots met so far */
#define EHR_LM_F_PRIOR 15    /* the prior's term of F_acc (ehr_lm_update_prior; never written without a prior) */
#define EHR_LM_THETA 16      /* [32] the accepted parameters */
#define EHR_LM_DELTA 48      /* [32] the last delta */
#define EHR_LM_G 80          /* [32] g_acc */
#define EHR_LM_H 112         /* [32][32] H_acc, row stride 32 */
#define EHR_LM_STATE_DOUBLES 1136
int ehr_lm_linearize(const float* dof, const float* K, const float* link_poses, int B, int L, int H, int W, float near_plane,
                     float far_plane, const float* joint_frames, const uint32_t* upstream, const int32_t* joint_kind,
                     const int32_t* free_list, int F, int J, int free4_mask, int tie_focal, int N, float* mvp, float* dmvp,
                     void* stream);
int ehr_lm_update(const double* info, const double* grad, const long long* count, const float* loss, int B, int N, float* dof,
                  float* offset, const int32_t* free_list, int F, int J, float* theta, int free4_mask, int tie_focal,
                  const float* K0, float* K, int H, int W, double ftol, double lambda_max, int finalize, double* state,
                  double* log, int log_rows, void* stream);

/* Levenberg-Marquardt with a Gaussian prior: the MAP estimate
 *     F(theta) = sum_views w (mask - ref)^2 + sum_k p_k (theta_k - mu_k)^2,     p_k = sigma2 / sigma_k^2  (the caller's),
 * for the solo update and the rig's.  prior_weight, prior_mean: [N] float64 device arrays in the parameter order of the state
 * block (the rig's: N = 6 C + F); p_k == 0 puts no prior on parameter k.  Both NULL: the call IS ehr_lm_update /
 * ehr_lm_update_rig, bit for bit (they are these entries called with NULL, NULL); one NULL and the other not: EHR_ERR_INVALID.
 * Everything else is the update's, with these additions, in this order (float64, -ffp-contract=off: no fused multiply-add):
 *   a. After step 1, at the trial (the parameters as the pointers hold them): d_k = (double) theta_k - mu_k,
 *      Fp = sum_k (p_k * d_k) * d_k for k ascending from 0.0; terms with p_k == 0 are skipped, not added.  A non-finite Fp, a
 *      non-finite mu_k where p_k != 0, or a p_k that is negative or not finite makes the call REPORTED (step 2; rig-wide).
 *   b. Step 3 judges F = F_data + Fp (one addition): EHR_LM_F and EHR_LM_F_TRIAL hold this total, the log's first column too.
 *      An accept stores Fp in EHR_LM_F_PRIOR: the data's loss at the accepted point is F_acc - F_prior.
 *   c. The stored linearisation (EHR_LM_H, EHR_LM_G, EHR_LM_THETA) stays the DATA'S: sum w J J^T and the data's gradient.
 *      Behind step 3, accepted or rejected, the system that is solved gets, for every k with p_k != 0,
 *          H[k][k] += p_k        g[k] += 2.0 * p_k * (theta_acc_k - mu_k),
 *      so a rejected call rebuilds exactly the system the accepting call solved.
 *   d. Steps 4-6 run on that system: the scaling is the posterior diagonal's, and a parameter WITHOUT data information but
 *      with p_k > 0 is no longer left out -- the prior alone pulls it towards mu_k (intended).  pred, ftol * F_acc,
 *      lambda_max and the float32-spacing rule are unchanged; restore, finalize and done likewise.
 * ehr_lm_update_multi has no such form (pose only; ehr_lm_update_multi_calib below takes [P,N] rows).  Out of scope: full prior covariances, N > EHR_LM_MAX_PARAMS.
 * ehr_version() is unchanged: the presence of these symbols is the capability check. */
int ehr_lm_update_prior(const double* info, const double* grad, const long long* count, const float* loss, int B, int N,
                        float* dof, float* offset, const int32_t* free_list, int F, int J, float* theta, int free4_mask,
                        int tie_focal, const float* K0, float* K, int H, int W, double ftol, double lambda_max, int finalize,
                        double* state, double* log, int log_rows, const double* prior_weight, const double* prior_mean,
                        void* stream);

/* Multi-start Levenberg-Marquardt: the two calls above for P hypotheses of ONE problem, so that an iteration of all of them is
 *     ehr_lm_linearize_multi -> ehr_mask_information (P*Bv views) -> ehr_lm_update_multi                    on one stream,
 * whatever P is.  Pose only: no joint offsets, no intrinsics (N = 6 tangents; the update takes N in 1..6 like the solo entry where
 * nothing but the pose is free).  Device pointers only; neither call allocates, synchronises or uses an atomic.  The contract is
 * ehr_solver_step_multi's: hypothesis p is, bit for bit, its solo solve -- both kernels call the device functions of the solo
 * kernels.
 *   ehr_lm_linearize_multi : virtual view b = p * Bv + j takes dof[p] and link_poses[j] (ehr_solver_step_multi's layout; K and
 *                            link_poses are shared, never copied).  mvp [P*Bv,L,16], dmvp [6,P*Bv,L,16]; views [p Bv, (p+1) Bv)
 *                            of both hold the bits ehr_lm_linearize(dof + 6 p, ..., B = Bv, F = 0, free4_mask = 0, N = 6) writes.
 *                            One thread per (k, b, l) matrix.
 *   ehr_lm_update_multi    : a grid of P workgroups of one wave.  Workgroup p runs steps 1-6 of ehr_lm_update on its own slices:
 *                            views [p Bv, (p+1) Bv) of info / grad / count / loss summed in view order, dof + 6 p,
 *                            state + p * EHR_LM_STATE_DOUBLES and log + p * log_rows * 4 (log may be NULL).  Reported, done and
 *                            finalize apply to ONE hypothesis: a non-finite sum or a count < 0 among hypothesis p's views discards
 *                            p's trial only; a hypothesis that is done only restores its accepted pose while the others move;
 *                            finalize != 0 restores all P accepted poses and changes nothing else.  The caller prepares every
 *                            state block as for ehr_lm_update.
 * Both refuse (EHR_ERR_INVALID) NULL tensors, P < 1, Bv < 1 and sizes whose matrix count overflows 32 bits; the update also N
 * outside 1..6.  Free joints or intrinsics per hypothesis: the _multi_calib entries below.  Out of scope: a shared-reference
 * form of ehr_mask_information (the caller tiles the reference), retiring finished hypotheses from the render.
 * ehr_version() is unchanged: the presence of these symbols is the capability check. */
int ehr_lm_linearize_multi(const float* dof, const float* K, const float* link_poses, int P, int Bv, int L, int H, int W,
                           float near_plane, float far_plane, float* mvp, float* dmvp, void* stream);
int ehr_lm_update_multi(const double* info, const double* grad, const long long* count, const float* loss, int P, int Bv, int N,
                        float* dof, double ftol, double lambda_max, int finalize, double* state, double* log, int log_rows,
                        void* stream);

/* Multi-start Levenberg-Marquardt with joint offsets, intrinsics and priors per hypothesis: P hypotheses
 * of ONE problem that each own a FULL parameter set, so that an iteration of all of them is
 *     [ehr_joint_forward_multi, if joints are free] -> ehr_lm_linearize_multi_calib -> ehr_mask_information (P*Bv views)
 *                                                   -> ehr_lm_update_multi_calib                                on one stream.
 * Everything that can differ between hypotheses is a per-hypothesis array -- dof [P,6], offset [P,J], theta [P,4], K [P,9],
 * link_poses [P*Bv,L,16], joint_frames [P*Bv,J,6], prior_weight / prior_mean [P,N] -- one layout, no "shared or not" flags; the
 * joint table, free_list and K0 describe the problem and are shared.  The parameters' order, F, J, free4_mask, tie_focal and N
 * are ehr_lm_linearize's.  Device pointers only; no call allocates, synchronises or uses an atomic.  The contract: hypothesis p
 * is, bit for bit, its solo solve -- every kernel calls the device functions of its solo kernel.
 *   ehr_joint_forward_multi      : a grid of P*Bv workgroups of one wave; virtual view b = p * Bv + j walks qpos[j] + offset[p]
 *                                  (qpos [Bv,J] float64, offset [P,J] float32).  Block p of link_poses / joint_frames holds the
 *                                  bytes ehr_joint_forward(..., qpos, offset + p J, B = Bv) writes.
 *   ehr_lm_linearize_multi_calib : one thread per (k, b, l) matrix, k in [-1, N); view b of hypothesis p = b / Bv takes dof + 6 p,
 *                                  K + 9 p, link_poses[b] and joint_frames[b] (NULL where F == 0).  mvp [P*Bv,L,16], dmvp
 *                                  [N,P*Bv,L,16]; views [p Bv, (p+1) Bv) of both hold the bits ehr_lm_linearize writes for
 *                                  hypothesis p's rows with B = Bv.
 *   ehr_lm_update_multi_calib    : a grid of P workgroups of one wave.  Workgroup p runs ehr_lm_update -- or, with prior_weight
 *                                  and prior_mean given, ehr_lm_update_prior on rows p of them -- on its own slices: views
 *                                  [p Bv, (p+1) Bv), dof + 6 p, offset + J p, theta + 4 p, K + 9 p (offset / theta, K0, K: NULL
 *                                  where F == 0 / free4_mask == 0), state + p * EHR_LM_STATE_DOUBLES, log + p * log_rows * 4.
 *                                  Reported, done and finalize apply to ONE hypothesis, as for ehr_lm_update_multi; with F == 0
 *                                  and free4_mask == 0 and no prior it writes ehr_lm_update_multi's bytes.
 * All refuse (EHR_ERR_INVALID) NULL tensors, P < 1, Bv < 1, an N that is not 6 + F + the free intrinsics (the update also takes
 * N in 1..5 where nothing but the pose is free), N > EHR_LM_MAX_PARAMS and sizes whose matrix count overflows 32 bits; the update
 * refuses prior_weight and prior_mean given singly.  Out of scope: rigs, retiring finished hypotheses from the render, a
 * shared-reference form of ehr_mask_information.
 * ehr_version() is unchanged: the presence of these symbols is the capability check. */
int ehr_joint_forward_multi(const int32_t* parent, const double* origin, const int32_t* kind, const double* axis,
                            const int32_t* qidx, const int32_t* use, int N, int J, int L, const double* qpos,
                            const float* offset, int P, int Bv, float* link_poses, float* joint_frames, void* stream);
int ehr_lm_linearize_multi_calib(const float* dof, const float* K, const float* link_poses, int P, int Bv, int L, int H, int W,
                                 float near_plane, float far_plane, const float* joint_frames, const uint32_t* upstream,
                                 const int32_t* joint_kind, const int32_t* free_list, int F, int J, int free4_mask,
                                 int tie_focal, int N, float* mvp, float* dmvp, void* stream);
int ehr_lm_update_multi_calib(const double* info, const double* grad, const long long* count, const float* loss, int P, int Bv,
                              int N, float* dof, float* offset, const int32_t* free_list, int F, int J, float* theta,
                              int free4_mask, int tie_focal, const float* K0, float* K, int H, int W, double ftol,
                              double lambda_max, int finalize, double* state, double* log, int log_rows,
                              const double* prior_weight, const double* prior_mean, void* stream);

/* Eye-in-hand: the camera is bolted to node `mount` of the joint table instead of standing in the base frame (DESIGN.md section
 * 6w).  The unknown pose is X = T_cam<-mount, and the camera<-link transform of view b and rendered link l is
 * X @ inv(F_m(b)) @ F_l(b), with F_i the base-frame frames ehr_joint_forward walks.  These two entries are ehr_joint_forward and
 * ehr_joint_forward_multi with that change of frame: the same walk (one wave per view, the same LDS frames, the same float64
 * arithmetic), then, in float64 from the LDS frames and rounded to float32 ONCE:
 *   link_poses[b,l]   : R = R_m^T R_u, entry (r,c) = (R_m[0][r] R_u[0][c] + R_m[1][r] R_u[1][c]) + R_m[2][r] R_u[2][c];
 *                       t = R_m^T (t_u - t_m), the difference first, entry r = (R_m[0][r] d[0] + R_m[1][r] d[1]) + R_m[2][r] d[2];
 *                       the last row is F_u's.  u = use[l]; a `use` out of range gives NaN, as in ehr_joint_forward.
 *   joint_frames[b,j] : a' = sigma_j R_m^T a_j and p' = R_m^T (p_j - t_m), the products associated as above; a_j (float64, not
 *                       yet rounded) and p_j are ehr_joint_forward's axis and point; sigma_j = -1 where bit j of mount_upstream
 *                       is set (active joint j lies between the root and the mount) and +1 otherwise.
 * With these, and with the mask  upstream[l] XOR mount_upstream  in place of upstream[l], the derivative formula of
 * ehr_joint_backward_adam, D = [ [a']x R | a' x (t - p') ; 0 0 ] (prismatic [ 0 | a' ; 0 0 ]), is d(inv(F_m) F_l)/d offset_j,
 * since that derivative is (u_l(j) - u_m(j)) [xi'_j]^ inv(F_m) F_l and D is linear in a'.  ehr_joint_backward_adam,
 * ehr_lm_linearize, ehr_lm_linearize_multi_calib, ehr_mask_information and the LM updates therefore serve a mounted camera
 * unchanged.  With mount = the root (identity frame, mount_upstream = 0) the outputs equal ehr_joint_forward's in value (the
 * sign of a zero may differ).  Both refuse (EHR_ERR_INVALID) what their unmounted twins refuse and a mount outside [0, N).
 * No atomics, no allocation; bit-reproducible; capturable.  The multi form has ehr_joint_forward_multi's virtual-view layout, and
 * block p of its outputs holds the bytes ehr_joint_forward_mounted(..., qpos, offset + p J, B = Bv) writes.
 * Out of scope: camera rigs (ehr_rig_backward_adam takes one `upstream` for all cameras).
 * ehr_version() is unchanged: the presence of these symbols is the capability check. */
int ehr_joint_forward_mounted(const int32_t* parent, const double* origin, const int32_t* kind, const double* axis,
                              const int32_t* qidx, const int32_t* use, int N, int J, int L, int mount, uint32_t mount_upstream,
                              const double* qpos, const float* offset, int B, float* link_poses, float* joint_frames,
                              void* stream);
int ehr_joint_forward_multi_mounted(const int32_t* parent, const double* origin, const int32_t* kind, const double* axis,
                                    const int32_t* qidx, const int32_t* use, int N, int J, int L, int mount,
                                    uint32_t mount_upstream, const double* qpos, const float* offset, int P, int Bv,
                                    float* link_poses, float* joint_frames, void* stream);

/* Levenberg-Marquardt over a camera rig: C fixed cameras watch one arm and share its joint offsets (ehr_rig_backward_adam's
 * setting), solved as ONE system of N = 6 C + F <= EHR_LM_MAX_PARAMS parameters in the order of
 * easyhec_amd.information.rig_information: cam0.dof[0..5], cam1.dof[0..5], ..., then offset[free_list[0..F)].  One iteration is
 *     per camera c : ehr_joint_forward (qpos_c, the SHARED offsets) -> ehr_lm_linearize (camera c's dof, K, link_poses,
 *                    joint_frames; N_c = 6 + F) -> ehr_mask_information on camera c's context
 *                    -> info_c [B_c,N_c,N_c], grad_c [B_c,N_c], count_c [B_c], loss_c [B_c]
 *     once         : ehr_lm_update_rig                                                                      on one stream.
 * The three per-camera calls are used as they are.  `cams` is a HOST array of C structs of device pointers: it is validated
 * here (EHR_ERR_INVALID for a NULL pointer, B_c < 1, C < 1 or N > EHR_LM_MAX_PARAMS) and travels to the kernel by value.  One
 * workgroup of one wave, float64, fixed order, no atomics; never allocates or synchronises.  The state block, the log and
 * ftol / lambda_max / finalize are ehr_lm_update's.  In order:
 *   1. Per camera, in camera order: S_c = sum_b info_c[b], s_c = sum_b grad_c[b], F_c = sum_b (double) loss_c[b],
 *      n_c = sum_b count_c[b], each from 0.0 in view order (ehr_lm_update's sums).  H and g are cleared, then every camera is
 *      embedded in camera order, each entry `+=`: local index i < 6 -> 6 c + i, local 6 + f -> 6 C + f.  A pose-pose and a
 *      pose-offset block so has one term, the offset-offset block C terms in camera order, and the block between two different
 *      cameras' poses stays 0.0.  F = F_0 + F_1 + ..., count = n_0 + n_1 + ... in camera order, from 0.0.  With C == 1 every
 *      value is ehr_lm_update's, bit for bit.
 *   2. A non-finite sum or loss or a count < 0 of ANY camera reports the call for the whole rig: every camera's accepted pose
 *      and the accepted offsets are written back, `reported` is incremented, nothing else moves (ehr_rig_backward_adam's all or
 *      nothing).
 *   3-6. ehr_lm_update's, by the same device function over the rig's parameters: accept or reject, the damped scaled Cholesky
 *      solve with the exclusion of H_kk <= 0 and the retries, pred, the stopping rule and the trial fl32(theta_acc + delta)
 *      through every cams[c].dof and offset.  There are no intrinsics in a rig: no K is rewritten.
 * Out of scope here: per-camera intrinsics, more than EHR_LM_MAX_PARAMS parameters (C <= 5 with F <= 2, C <= 4 with F <= 8, ...);
 * ehr_lm_update_rig_arrow below takes both.
 * ehr_version() is unchanged: the presence of this symbol is the capability check. */
typedef struct {            /* one camera of the rig's update; all pointers are device pointers */
    const double *info, *grad;  const long long* count;  const float* loss;   /* ehr_mask_information's outputs for its views */
    float* dof;                                                                 /* its 6 pose coordinates */
    int B;
} ehr_lm_rig_camera;
int ehr_lm_update_rig(const ehr_lm_rig_camera* cams /* HOST array [C] */, int C, float* offset, const int32_t* free_list, int F,
                      int J, double ftol, double lambda_max, int finalize, double* state, double* log, int log_rows,
                      void* stream);
/* The rig's update under a Gaussian prior: see ehr_lm_update_prior; prior_weight, prior_mean [6 C + F] in the rig's order. */
int ehr_lm_update_rig_prior(const ehr_lm_rig_camera* cams /* HOST array [C] */, int C, float* offset, const int32_t* free_list,
                            int F, int J, double ftol, double lambda_max, int finalize, double* state, double* log,
                            int log_rows, const double* prior_weight, const double* prior_mean, void* stream);

/* The rig's Levenberg-Marquardt update on its BLOCK-ARROW system: per-camera intrinsics, and no limit of 32 parameters.
 * Camera c frees I_c in 0..4 intrinsics (free4_mask / tie_focal as for ehr_lm_linearize; the set may differ per camera and may
 * be empty), P_c = 6 + I_c, base_c = P_0 + ... + P_{c-1}, S0 = base_C, N = S0 + F, in the order
 *     cam0.dof[0..5], cam0.theta[...], cam1.dof[0..5], cam1.theta[...], ..., offset[free_list[0..F)]
 * with theta[...] in ehr_lm_linearize's order (f | fx, fy, then cx, cy).  Without intrinsics it is ehr_lm_update_rig's order.
 * The per-camera calls are unchanged: ehr_joint_forward, ehr_lm_linearize and ehr_mask_information with the camera's own
 * free4_mask, tie_focal and N_c = 6 + F + I_c; camera c's local index (dof, offsets, intrinsics) embeds as
 *     i < 6 -> base_c + i,     6 + f -> S0 + f,     6 + F + q -> base_c + 6 + q.
 * Limits: 1 <= C <= EHR_LM_ARROW_MAX_CAMERAS, F + I_c <= EHR_LM_ARROW_MAX_SHARED (N_c <= 32), hence N <= 182.
 * `cams` is a HOST array, judged here before anything is launched (EHR_ERR_INVALID, the message names the camera: C outside
 * 1..16, a NULL pointer, B_c < 1, F + I_c > 26, free4_mask outside 0..15, tie_focal without bits 0 and 1, a free mask with NULL
 * theta / K0 / K, one prior pointer NULL and the other not) and travels to the kernel by value.  One workgroup of 256 threads,
 * float64, every sum in a fixed order, no atomics, every loop bounded; never allocates or synchronises.
 *   1. ehr_lm_update_rig's head: per camera, in camera order, S_c, s_c, F_c, n_c from 0.0 in view order; the system is cleared
 *      and every camera embedded with `+=` in camera order (the shared corner gets its C terms one camera at a time, by one owner
 *      per entry); F and count from 0.0 in camera order.  The matrices need not be symmetric to the last bit: both halves of
 *      every block are stored as given.
 *   2, 3. ehr_lm_update's: a bad sum of ANY camera reports the call rig-wide (every accepted pose, every accepted theta with its
 *      K rewritten, and the accepted offsets are written back, `reported` is incremented, nothing else moves); accept / reject
 *      and Nielsen's schedule.  prior_weight, prior_mean [N] (both or neither): ehr_lm_update_prior's rule -- the term joins F,
 *      p_k and 2 p_k (theta_acc_k - mu_k) the system that is solved, the stored H, g stay the data's.
 *   4. (S H S + lambda I) y = -S g / 2, parameters with H_kk <= 0 left out, by block elimination in the system's order: for
 *      c = 0 .. C-1, A_c = L_c L_c^T (right-looking, column by column), W_c = L_c^-1 B_c, z_c = L_c^-1 r_c; the corner and its
 *      right-hand side lose W_c^T W_c and W_c^T z_c, the terms in camera order and within a camera in row order k = 0 .. P_c-1;
 *      S^ = L_s L_s^T, y_s by two triangular solves, y_c = L_c^-T (z_c - W_c y_s).  This is the dense right-looking Cholesky of
 *      ehr_lm_update in the system's order with the updates by structurally zero blocks left out.  A non-positive or non-finite
 *      pivot anywhere raises lambda like a rejection and factors again, 8 times at the most, then why = 4.  (S H S) y per row
 *      over that row's structurally non-zero columns, ascending; pred, the stopping rule and `small` for k ascending over N.
 *   6. The trial fl32(theta_acc + delta) through every cams[c].dof, every free theta element (under tie_focal theta[1] follows
 *      theta[0]) and offset; every camera with free intrinsics gets its K rewritten from K0 and theta by
 *      ehr_intrinsics_backward_adam's "writing K" rule; a camera without has its K left untouched.
 * The state block has EHR_LM_ARROW_STATE_DOUBLES float64; the caller clears it and sets EHR_LM_LAMBDA and EHR_LM_NU.  Words
 * 0..15 are EHR_LM_LAMBDA .. EHR_LM_F_PRIOR; then theta, delta, g with a capacity of EHR_LM_ARROW_MAX_PARAMS each; then H_acc
 * packed, every offset a constant: per camera c at EHR_LM_ARROW_H + c * EHR_LM_ARROW_CAMERA_STRIDE a panel [10][10 + 26] (row i
 * of its block: columns 0..P_c-1 the block, columns 10 + f its coupling to offset f) followed at EHR_LM_ARROW_BORDER_T by the
 * border's other half [26][10] (row f, column i: H[S0 + f][base_c + i]); then the corner [26][26] at EHR_LM_ARROW_CORNER.
 * ehr_version() is unchanged: the presence of this symbol is the capability check. */
#define EHR_LM_ARROW_MAX_CAMERAS 16
#define EHR_LM_ARROW_MAX_BLOCK 10      /* P_c <= 6 + 4 */
#define EHR_LM_ARROW_MAX_SHARED 26     /* F + I_c <= 26 */
#define EHR_LM_ARROW_MAX_PARAMS 192    /* capacity of theta, delta, g (N <= 182) */
#define EHR_LM_ARROW_THETA 16
#define EHR_LM_ARROW_DELTA 208
#define EHR_LM_ARROW_G 400
#define EHR_LM_ARROW_H 592
#define EHR_LM_ARROW_PANEL_STRIDE 36   /* row stride of a camera's panel */
#define EHR_LM_ARROW_BORDER_T 360      /* within a camera's part: the border's other half, row stride 10 */
#define EHR_LM_ARROW_CAMERA_STRIDE 620
#define EHR_LM_ARROW_CORNER 10512      /* [26][26], row stride 26 */
#define EHR_LM_ARROW_STATE_DOUBLES 11188
typedef struct {            /* one camera of the arrow update; all pointers are device pointers */
    const double *info, *grad;  const long long* count;  const float* loss;   /* ehr_mask_information's outputs, N_c = 6 + F + I_c */
    float* dof;                                                                 /* its 6 pose coordinates */
    float* theta;  const float* K0;  float* K;                                  /* NULL where free4_mask == 0 */
    int B, H, W, free4_mask, tie_focal;
} ehr_lm_rig_arrow_camera;
int ehr_lm_update_rig_arrow(const ehr_lm_rig_arrow_camera* cams /* HOST array [C] */, int C, float* offset,
                            const int32_t* free_list, int F, int J, double ftol, double lambda_max, int finalize, double* state,
                            double* log, int log_rows, const double* prior_weight, const double* prior_mean /* [N] */,
                            void* stream);

/* Information-gain exploration: which candidate joint configuration to observe next. A candidate is a group of S consecutive
 * views of info [Q,S,N,N] -- ehr_mask_information's matrices of the views the candidate WOULD give (the op's info does not depend
 * on the reference mask, so they exist before the candidate is observed); S > 1 averages over sampled poses or sums over cameras.
 * Both calls take device pointers only, never allocate or synchronise and launch on `stream`; k rounds of gain + pick are 2k
 * launches with no host round trip.  No atomics; every sum in a fixed order.  1 <= N <= EHR_IG_MAX_PARAMS, Q >= 1, S >= 1.
 *   ehr_information_gain : A [N,N] float64 = what is already known (a prior plus the frames so far), symmetric, with a finite
 *                          diagonal > 0 (otherwise EVERY gain is NaN).  H_q = scale * (info[q,0] + info[q,1] + ...), summed in
 *                          view order; X0 = A, X1 = A + H_q.  Both are scaled by s_i = 1 / sqrt(A_ii) as (x_ij s_i) s_j and factored
 *                          by Cholesky in float64; ld(X) = 2 sum_j log r_jj.  Where interest_mask (bit k: parameter k is of
 *                          interest) does not cover all N bits, the same quantity of the sub-matrix on the COMPLEMENT indices
 *                          (ascending) is subtracted: the log-determinant of the MARGINAL information of the parameters of
 *                          interest, logdet X - logdet X_bb.  gain[q] = ld(X1) - ld(X0), both by the same device function in the
 *                          same wave: a candidate whose H_q is all zeros gets exactly +0.0.  valid[q] == 0 (valid may be NULL)
 *                          or taken[q] != 0 (taken may be NULL): gain = -inf, and that candidate's info is not read.  A
 *                          non-finite entry of H_q or a pivot that is not positive: NaN (this is how a reported
 *                          ehr_mask_information call surfaces).  A gain depends on A and the candidate's own matrices alone: the
 *                          same bits alone, in any batch, at any position.  One wave per candidate.
 *   ehr_information_pick : one workgroup.  q* = the lowest index among the candidates with the largest FINITE gain (NaN and -inf
 *                          never win).  None: picked[round] = -1, picked_gain[round] = NaN, A and taken untouched.  Otherwise
 *                          picked[round] = q*, picked_gain[round] = gain[q*], taken[q*] = 1 and A[e] = A[e] + H_q*[e] entry by
 *                          entry, H_q* by the expression above (a product rounded, then a sum rounded): A stays exactly symmetric
 *                          where the matrices are.
 * ehr_version() is unchanged: the presence of these symbols is the capability check. */
#define EHR_IG_MAX_PARAMS 32
int ehr_information_gain(const double* A, const double* info, const int32_t* valid, const int32_t* taken, int Q, int S, int N,
                         double scale, uint32_t interest_mask, double* gain, void* stream);
int ehr_information_pick(const double* gain, const double* info, int Q, int S, int N, double scale, int round, double* A,
                         int32_t* taken, int32_t* picked, double* picked_gain, void* stream);

/* Feasibility of candidate joint configurations on sphere proxies (easyhec_amd/feasibility.py, csrc/ehr_feasible.hip): the
 * clearance of every configuration against itself, against planes and obstacle spheres, and inside a ball of allowed reach.
 * Static and conservative: where the proxy spheres cover the meshes, clear spheres mean clear meshes.  Device pointers but for
 * sphere_offsets, a HOST array that travels in the kernel's arguments (it sizes the launch's LDS and is checked here, with no
 * read-back); never allocates or synchronises, no atomics; one launch on `stream`.
 *   link_poses [n,L,16] float32 as ehr_joint_forward writes them; spheres [S,4] float64 = link-frame centre and radius, the
 *   links concatenated, link l's being sphere_offsets[l] .. sphere_offsets[l+1] ([L+1] int32 on the HOST, ascending from 0 to S);
 *   link_bounds [L,4] float64 = one link-frame sphere per link that CONTAINS every sphere of the link (used for culling only);
 *   pair_enable [L] uint32: bit j of word i (j > i) = link pair (i,j) is checked; planes [Np,4] float64 (n, d): n.x + d >= 0 is
 *   inside, n of unit length (a longer one would let a link's bound cull what it should not), Np <= EHR_FEAS_MAX_PLANES (may be NULL when 0); obstacles [No,4] float64 spheres in the base frame, No <=
 *   EHR_FEAS_MAX_OBSTACLES (may be NULL when 0); env_links: bit l = link l is tested against planes and obstacles; reach [4]
 *   float64 = centre o and radius R of the allowed ball, or NULL.
 * Arithmetic: float64 throughout, every operation rounded on its own (no contraction), the pose entries widened to double:
 *   world centre     c_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k          (k = 0..2; the sphere keeps its radius)
 *   sphere / sphere  sqrt((dx dx + dy dy) + dz dz) - (r_a + r_b)       (also sphere / obstacle; d = c_a - c_b)
 *   plane            (((n_x c_x + n_y c_y) + n_z c_z) + d) - r
 *   reach            R - (sqrt((dx dx + dy dy) + dz dz) + r)           (d = c - o)
 * Outputs, [n] each: self_clear = min(cutoff, min over the sphere pairs of every enabled link pair); env_clear = min(cutoff,
 * min over planes and obstacles for the spheres of the links in env_links); reach_clear = min(cutoff, min over all spheres),
 * cutoff where reach is NULL; self_pair = 32 i + j of the lowest-numbered enabled pair that attains self_clear, -1 where nothing
 * lies below cutoff.  No pairs, no planes and obstacles, or no spheres: cutoff.  min is exact in any order: the results do not
 * depend on the reduction's shape.  A configuration with a pose entry that is not finite gets NaN in all three clearances and
 * self_pair -1 (a filter that cannot judge must not pass), and leaves its neighbours untouched.  A link pair, or a link against
 * a plane or an obstacle, is skipped through link_bounds only where the bound exceeds cutoff + 1e-6: rounding in the bound
 * never changes an output.  Refused (EHR_ERR_INVALID): L outside 1..EHR_FEAS_MAX_LINKS, S > EHR_FEAS_MAX_SPHERES, n < 1, n_planes
 * or n_obstacles out of range, offsets that do not ascend from 0, cutoff not finite or <= 0, and a device whose LDS cannot hold
 * the S spheres (32 bytes each).  The spheres, bounds, planes and obstacles are device memory: finite values are the caller's
 * to ensure (a NaN among them is ignored by the minimum, not reported).
 * ehr_version() is unchanged: the presence of the symbol is the capability check. */
#define EHR_FEAS_MAX_LINKS 32
#define EHR_FEAS_MAX_SPHERES 4096
#define EHR_FEAS_MAX_PLANES 16
#define EHR_FEAS_MAX_OBSTACLES 1024
int ehr_config_clearance(const float* link_poses, const double* spheres, const int32_t* sphere_offsets, const double* link_bounds,
                         const uint32_t* pair_enable, const double* planes, int n_planes, const double* obstacles,
                         int n_obstacles, uint32_t env_links, const double* reach, double cutoff, int n, int L,
                         double* self_clear, int32_t* self_pair, double* env_clear, double* reach_clear, void* stream);

/* The meshes behind the sphere proxies (easyhec_amd/feasibility.py, csrc/ehr_mesh_clearance.hip): per configuration the exact
 * distance between the triangle meshes of the enabled link pairs, and of the meshes to planes and obstacle spheres.  The proxy
 * spheres are the broad phase, the triangles each of them stands for the narrow one.  Inputs as ehr_config_clearance's (the
 * same limits; no reach), device pointers but for sphere_offsets, and
 *   triangles [T,9] float64: link-frame corner coordinates (x y z of corner 0, 1, 2), ordered so that the triangles of proxy
 *   sphere s are tri_offsets[s] .. tri_offsets[s+1]; tri_offsets [S+1] int32 on the DEVICE, ascending from 0 to T (nobody reads
 *   it back: the kernel clamps every range into 0..T, so a wrong table gives wrong answers, not wild reads); T <=
 *   EHR_MESH_MAX_TRIANGLES; pair_enable as above, the MESH pair list.  Every triangle of sphere s must lie inside that sphere,
 *   and every sphere of a link inside link_bounds: they cull.
 * Arithmetic: float64 throughout, every operation rounded on its own, division and square root correctly rounded, the pose
 * entries widened to double.  With u.v = (u_x v_x + u_y v_y) + u_z v_z, u x v = (u_y v_z - u_z v_y, u_z v_x - u_x v_z,
 * u_x v_y - u_y v_x), |u|^2 = (u_x u_x + u_y u_y) + u_z u_z, clamp(x) = 0 if x < 0, 1 if x > 1, else x, and ratio(p, q) = p / q
 * if q > 0, else 0 (the exact-zero test of a zero-length edge or a zero-area triangle: nothing divides by 0, no epsilon):
 *   world corner      w_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k                        (as a sphere's centre)
 *   point / segment   P(p; a,b): ab = b - a, e = ab.ab, t = clamp((p - a).ab / e) if e > 0 else 0, q = a + ab t (per
 *                     coordinate a_x + ab_x t); |p - q|^2
 *   point / triangle  D(p; a,b,c): ab = b - a, ac = c - a, n = ab x ac.  If not n.n > 0 (zero area): min(P(p;a,b), P(p;b,c),
 *                     P(p;c,a)).  Else with ap = p - a, bp = p - b, cp = p - c, d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp,
 *                     d5 = ab.cp, d6 = ac.cp, vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, the first that holds of
 *                       d1 <= 0 and d2 <= 0                        (v, w) = (0, 0)
 *                       d3 >= 0 and d4 <= d3                       (1, 0)
 *                       vc <= 0 and d1 >= 0 and d3 <= 0            (ratio(d1, d1 - d3), 0)
 *                       d6 >= 0 and d5 <= d6                       (0, 1)
 *                       vb <= 0 and d2 >= 0 and d6 <= 0            (0, ratio(d2, d2 - d6))
 *                       va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0  w = ratio(d4 - d3, (d4 - d3) + (d5 - d6)), v = 1 - w
 *                       otherwise (the face)                       s = (va + vb) + vc, (ratio(vb, s), ratio(vc, s))
 *                     q = (a + ab v) + ac w per coordinate; |p - q|^2
 *   segment / segment E(p1,q1; p2,q2): d1 = q1 - p1, d2 = q2 - p2, r = p1 - p2, a = d1.d1, e = d2.d2, f = d2.r, c = d1.r,
 *                     b = d1.d2.  If a > 0 and e > 0: den = a e - b b, s = clamp((b f - c e) / den) if den > 0 else 0,
 *                     t = (b s + f) / e; if t < 0: t = 0, s = clamp(-c / a); else if t > 1: t = 1, s = clamp((b - c) / a).
 *                     Else if a > 0: t = 0, s = clamp(-c / a); else if e > 0: s = 0, t = clamp(f / e); else s = t = 0.
 *                     |(p1 + d1 s) - (p2 + d2 t)|^2
 *   piercing          X(p,q; a,b,c): n = (b - a) x (c - a), sp = n.(p - a), sq = n.(q - a); false unless (sp > 0 and sq < 0) or
 *                     (sp < 0 and sq > 0); with d = q - p, pa = a - p, pb = b - p, pc = c - p, u = d.(pa x pb), v = d.(pb x pc),
 *                     w = d.(pc x pa): true iff u, v, w are all >= 0 or all <= 0.  (A zero-area triangle has n = 0 and is never
 *                     pierced; its own edges still pierce.)
 *   triangle pair     0 if X holds for any of the three edges of one against the other (six tests); else the minimum of D of
 *                     each corner against the other triangle (six) and E of each edge pair (nine; edge k runs from corner k to
 *                     corner (k + 1) mod 3).  An edge through the middle of a large triangle is far from all fifteen.
 *   plane             ((n_x w_x + n_y w_y) + n_z w_z) + d for a corner w;     obstacle   sqrt(D(centre; triangle)) - radius
 * Outputs, [n] each (mesh_tri [n,2]): mesh_clear = min(cutoff, sqrt(the least triangle-pair value over all triangle pairs of
 * all enabled link pairs)); mesh_pair = 32 i + j of A link pair that attains it and mesh_tri = A triangle pair (rows of
 * `triangles`, of link i and of link j) that attains it -- not the lowest: among ties, the penetrating poses' many zeros
 * included, any -- or -1 where nothing lies below cutoff; env_clear = min(cutoff, the least plane value over the corners and the
 * least obstacle value over the triangles of the links in env_links).  A configuration with a pose entry that is not finite
 * gets NaN clearances and -1 witnesses, and leaves its neighbours untouched.  Minima are exact in any order and what is culled
 * lies above the result, so the clearances do not depend on how the work is dealt out: tests/mesh_clearance_reference.py
 * restates the above in numpy and the kernel is compared bit for bit.  A leaf pair, a triangle against a leaf, a triangle pair, a
 * leaf against a plane or an obstacle is skipped only where the gap of the spheres around the two exceeds the bar (cutoff, or
 * the least distance found so far) by 1e-6, which covers the float32 pose being no exact rotation.
 * One launch on `stream`; never allocates or synchronises; no atomics to global memory.  Refused (EHR_ERR_INVALID): the limits
 * of ehr_config_clearance (L, S, n, planes, obstacles, sphere_offsets that do not ascend from 0, cutoff), T outside
 * 0..EHR_MESH_MAX_TRIANGLES, NULL tensors.
 * ehr_version() is unchanged: the presence of the symbol is the capability check. */
#define EHR_MESH_MAX_TRIANGLES 1048576
int ehr_mesh_clearance(const float* link_poses, const double* spheres, const int32_t* sphere_offsets, const double* link_bounds,
                       const uint32_t* pair_enable, const double* planes, int n_planes, const double* obstacles, int n_obstacles,
                       uint32_t env_links, double cutoff, int n, int L, const double* triangles, const int32_t* tri_offsets,
                       int n_triangles, double* mesh_clear, int32_t* mesh_pair, int32_t* mesh_tri, double* env_clear,
                       void* stream);

/* Certified clearance along the whole joint segment (easyhec_amd/feasibility.py, csrc/ehr_segment_clearance.hip): per candidate
 * either the sphere proxies keep more than `margin` on ALL of the straight joint-space segment q(t) = q0 + t d, d = q1 - q0, t in
 * [0,1], or how far the move is certified and what stopped it.  Bisection with conservative advancement; on the device,
 * conservative, one launch on `stream`, no atomics, no allocation, no host round trip.
 * Inputs: the kinematic table, offset [J] float32, N, J, L as ehr_joint_forward takes them; q0 [J], q1 [n,J] float64; spheres,
 * sphere_offsets (HOST), link_bounds, pair_enable, planes, obstacles, env_links, reach, cutoff as ehr_config_clearance takes them
 * (L <= EHR_FEAS_MAX_LINKS here too); upstream [L] uint32 (bit j: active joint j lies between the root and rendered link l);
 * joint_below [J] uint32 (bit k of word j: joint k lies strictly below joint j, i.e. j moves k's axis); reach_radius W [J,L] float64
 * (below); margin; the budget min_depth <= max_depth <= EHR_SEG_MAX_DEPTH, 1 <= max_evals <= EHR_SEG_MAX_EVALS.
 * Arithmetic: float64, every operation rounded on its own; a sum "over j" runs over ascending j and starts from 0.0.
 *   An evaluation at centre c with half-width h (dyadic, exact): q(c)_j = q0_j + c d_j; the kinematics of ehr_joint_forward at
 *   q(c) (offsets added inside, as there) give float32 link_poses and joint_frames (a_j, p_j); the spheres and link bounds go to
 *   the base frame by ehr_config_clearance's expression.  The RAW values self, self_pair, env, reach are those of
 *   ehr_joint_forward + ehr_config_clearance at q(c), bit for bit.
 *   lever arm      rho[j,s] = sqrt(|u|^2) + r_s, u = (c_s - p_j) x a_j = (v_y a_z - v_z a_y, v_z a_x - v_x a_z, v_x a_y - v_y a_x),
 *                  |u|^2 = (u_x u_x + u_y u_y) + u_z u_z, for a revolute joint j (a, p widened to double); 1 for any other
 *   W[j,l]         a bound, independent of the configuration, on the distance of any point of any proxy of link l from joint j's
 *                  axis: 0 where j is not upstream of l, 1 for a prismatic j (the host's; see feasibility.reach_radii)
 *   G[j,l]         sum over k in up(l) with k below j of |d_k| W[k,l]                              (once per candidate)
 *   C(l,M)         sum over j in M of |d_j| G[j,l]
 *   E_s            h * (sum over j in M of |d_j| rho[j,s]) + ((0.5 * h) * h) * C(l,M)               sphere s of link l under mask M
 *   Ebar(l,M)      h * (sum over j in M of |d_j| W[j,l]) + ((0.5 * h) * h) * C(l,M)                 >= every E_s of the link
 *   masks          link pair (a,b): up(a) & ~up(b) for a's spheres, up(b) & ~up(a) for b's (joints upstream of both move them
 *                  rigidly together); planes, obstacles and reach: up(l)
 * Why it holds: a point moves at most sum_j |d_j| dist(point, axis_j) per unit of t; that distance changes only through the
 * joints below j, by at most G[j,l] per unit of t; integrated over |t - c| <= h this is E_s.
 *   Certified values of [c - h, c + h], FEAS_CULL_SLACK = 1e-6 subtracted ONCE from each (the float32 rounding of poses and axes):
 *   cert_self  = min over the enabled pairs (a,b) with spheres on both links of: gap - (E_sa + E_sb) over the sphere pairs with
 *                gap < cutoff, and the pair's far value cutoff - (Ebar(a,Ma) + Ebar(b,Mb)), which stands for every sphere pair
 *                at or beyond cutoff (so a link pair culled through link_bounds changes no bit); cutoff where there is no pair
 *   cert_env   = min over the links of env_links with spheres (none if there are neither planes nor obstacles) of: value - E_s
 *                over the (sphere, plane) and (sphere, obstacle) values < cutoff, and the link's far value cutoff - Ebar(l,up(l))
 *   cert_reach = the same over all links with spheres and the reach values; cutoff where reach is NULL
 * Search: depth first, left to right, over the 2^min_depth dyadic intervals of [0,1].  For interval [a, a + 2h] of depth k,
 * evals counting this evaluation:
 *   1. a pose entry not finite: status 3.   2. raw fails (not self > margin, or not env > margin, or not reach >= 0): status 1 (hit).
 *   3. cert_self > margin, cert_env > margin and cert_reach >= 0: the three are folded into the running minima; next interval.
 *   4. k < max_depth and evals < max_evals: the two halves take the interval's place, the left one first.
 *   5. otherwise: status 2 (undecided).
 * No interval left: status 0 (clear).  evals == max_evals with intervals left after a certified one: status 2 with NaN stop values
 * (no evaluation stopped the search).  A q0 or q1 entry that is not finite: status 3 with evals 0.
 * Outputs [n]: status int32; t_free float64 = a at a stop (everything left of it is certified), 1 when clear; evals int32;
 * cert_self, cert_env, cert_reach = the minima over the certified intervals, cutoff if none; stop_self, stop_env, stop_reach,
 * stop_pair = the raw values of the evaluation that stopped the search (status 1, 2), NaN and -1 otherwise.  Optional trace
 * (both or neither NULL): trace_t [n,max_evals] = c and trace_val [n,max_evals,6] = raw self, env, reach, certified self, env,
 * reach (NaN for a status-3 evaluation) of every evaluation in order; entries past evals are untouched.  A candidate leaves its
 * neighbours untouched.
 * One workgroup of 256 threads per candidate, the spheres in LDS (40 bytes each).  Refused (EHR_ERR_INVALID): the limits of
 * ehr_joint_forward and ehr_config_clearance, S > EHR_SEG_MAX_SPHERES (what the 160 KiB of LDS of a gfx950 compute unit hold
 * beside the kinematics' frames), a budget outside its limits, margin outside 0 <= margin < cutoff, NULL tensors.
 * ehr_version() is unchanged: the presence of the symbol is the capability check. */
#define EHR_SEG_MAX_DEPTH 20
#define EHR_SEG_MAX_EVALS 4096
#define EHR_SEG_MAX_SPHERES 3264
int ehr_segment_clearance(const int32_t* parent, const double* origin, const int32_t* kind, const double* axis,
                          const int32_t* qidx, const int32_t* use, int N, int J, int L, const double* q0, const double* q1,
                          const float* offset, int n, const double* spheres, const int32_t* sphere_offsets,
                          const double* link_bounds, const uint32_t* pair_enable, const double* planes, int n_planes,
                          const double* obstacles, int n_obstacles, uint32_t env_links, const double* reach, double cutoff,
                          const uint32_t* upstream, const uint32_t* joint_below, const double* reach_radius, double margin,
                          int min_depth, int max_depth, int max_evals, int32_t* status, double* t_free, int32_t* evals,
                          double* cert_self, double* cert_env, double* cert_reach, double* stop_self, double* stop_env,
                          double* stop_reach, int32_t* stop_pair, double* trace_t, double* trace_val, void* stream);

/* The same certificate for the edges of a roadmap (easyhec_amd/feasibility.py, csrc/ehr_segment_clearance.hip; DESIGN.md section
 * 6v): edge e is the straight joint-space segment from node edge_a[e] to node edge_b[e].  One launch on `stream`, one workgroup
 * of 256 threads per edge, no atomics, no allocation, no host round trip.
 * Inputs: as ehr_segment_clearance takes them, but for q0, q1, n: nodes [V,J] float64, V, edge_a, edge_b [n] int32 (device).
 * Outputs: those of ehr_segment_clearance [n] and length [n] float64.
 *   Index out of range (edge_a[e] or edge_b[e] outside 0..V-1): status 3, evals 0, t_free 0, cert_self = cert_env = cert_reach =
 *   cutoff, stop_self = stop_env = stop_reach = NaN, stop_pair -1, length NaN; no node row is read and the edge's trace row is
 *   untouched.  This is how a caller marks an edge of a fixed-shape list "skipped" (-1).
 *   Valid edge: every output and every trace entry is, bit for bit, what ehr_segment_clearance gives as a one-candidate call with
 *   q0 = nodes[edge_a[e]], q1 = nodes[edge_b[e]] and the other arguments unchanged -- the same reach_radius, the same status 3 with
 *   evals 0 for a node entry that is not finite.
 *   length[e] = sqrt(sum over j of d_j * d_j), j ascending from 0.0, every operation rounded on its own, d_j = nodes[b][j] -
 *   nodes[a][j] (the d of the search); NaN where an entry of either node is not finite.
 * An edge leaves its neighbours untouched.  Refused (EHR_ERR_INVALID): what ehr_segment_clearance refuses, V < 1, NULL nodes,
 * edge_a, edge_b or length.
 * ehr_version() is unchanged: the presence of the symbol is the capability check. */
int ehr_edge_clearance(const int32_t* parent, const double* origin, const int32_t* kind, const double* axis, const int32_t* qidx,
                       const int32_t* use, int N, int J, int L, const double* nodes, int V, const int32_t* edge_a,
                       const int32_t* edge_b, const float* offset, int n, const double* spheres, const int32_t* sphere_offsets,
                       const double* link_bounds, const uint32_t* pair_enable, const double* planes, int n_planes,
                       const double* obstacles, int n_obstacles, uint32_t env_links, const double* reach, double cutoff,
                       const uint32_t* upstream, const uint32_t* joint_below, const double* reach_radius, double margin,
                       int min_depth, int max_depth, int max_evals, int32_t* status, double* t_free, int32_t* evals,
                       double* cert_self, double* cert_env, double* cert_reach, double* stop_self, double* stop_env,
                       double* stop_reach, int32_t* stop_pair, double* length, double* trace_t, double* trace_val, void* stream);

/* Single-source shortest paths of at most H edges over the usable edges of a roadmap (csrc/ehr_roadmap.hip).
 * One launch of ONE workgroup of 256 threads on `stream`, float64, no atomics, no allocation, no host round trip.
 * Inputs (device): a CSR adjacency adj_start [V+1], adj_node [A], adj_edge [A] int32 -- the slots of node v are adj_start[v] ..
 * adj_start[v+1] - 1, slot i leads to node adj_node[i] over edge adj_edge[i]; A is the number of slots the two arrays hold, and a
 * slot index outside 0..A-1 is not read; edge_status [E] int32, edge_length [E] float64 (ehr_edge_clearance's); 1 <= V <=
 * EHR_ROADMAP_MAX_NODES, E, source in 0..V-1, 1 <= H <= EHR_ROADMAP_MAX_HOPS.
 * Layers: D_0[v] = +inf, D_0[source] = 0.  Round r = 1..H, for every v: best = D_{r-1}[v], "carried"; over the slots i of v in
 * ascending order, u = adj_node[i], e = adj_edge[i]: the slot is skipped unless 0 <= u < V, 0 <= e < E, edge_status[e] == 0 and
 * edge_length[e] is finite and >= 0; c = D_{r-1}[u] + edge_length[e]; if c < best (strictly) then best = c and (u, e) is round
 * r's predecessor of v.  D_r[v] = best.  All H rounds always run.  Among equal lengths the lowest slot wins.
 * Outputs: dist [H+1,V] float64 = the layers; pred_node, pred_edge [H,V] int32 = round r's predecessor at row r-1, -1 where
 * carried; changed [H] int32 = the nodes that improved in each round (changed[H-1] == 0: any larger H gives the same answer);
 * hops [V], path [V,H+1] and path_edge [V,H] int32: the path of v, source first, -1 past its end, found by walking from (r = H,
 * x = v): while x's predecessor at r is "carried", r--; record it, go to the predecessor node, r--; until x == source.  hops is 0
 * for the source and -1, with a path of -1 throughout, for a node the walk does not bring to the source.  dist[H,v] is the
 * left-to-right float sum of edge_length along path_edge[v].
 * Refused (EHR_ERR_INVALID): V, H outside their limits, E < 0, A < 0, source outside 0..V-1, NULL tensors (adj_node, adj_edge may be
 * NULL when A == 0, edge_status and edge_length when E == 0).
 * ehr_version() is unchanged: the presence of the symbol is the capability check. */
#define EHR_ROADMAP_MAX_NODES 4096
#define EHR_ROADMAP_MAX_HOPS 8
int ehr_roadmap_paths(const int32_t* adj_start, const int32_t* adj_node, const int32_t* adj_edge, int A,
                      const int32_t* edge_status, const double* edge_length, int V, int E, int source, int H, double* dist,
                      int32_t* pred_node, int32_t* pred_edge, int32_t* hops, int32_t* path, int32_t* path_edge, int32_t* changed,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EHR_H */
