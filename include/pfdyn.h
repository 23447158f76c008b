/* pfdyn.h -- C ABI of libpfdyn.so: the MI355X (gfx950) implementation of PharmacoForge's
 * per-timestep denoising network and reverse-diffusion loop.
 *
 * Boundary replaced (reference = eflynn8/pharmacophore-diffusion, paths relative to its root):
 *   pharmacoforge/models/dynamics_gvp.py:131-185   PharmRecDynamicsGVP.forward   -> pf_dynamics_forward
 *   pharmacoforge/models/dynamics_gvp.py:187-246   add/remove_pharm_edges        -> inside pf_dynamics_forward
 *                                                                                  (pf_debug_get_edges exposes them)
 *   pharmacoforge/models/pharmacodiff.py:380-431   sample_p_zs_given_zt          -> pf_denoise_step
 *   pharmacoforge/models/pharmacodiff.py:433-488   sample_given_receptor (loop)  -> pf_sample
 *   pharmacoforge/models/pharmacodiff.py:88-108    com_removal                   -> inside pf_denoise_step / pf_sample
 *   pharmacoforge/dataset/protein_pharm_dataset.py:234-236  static pp radius graph -> pf_build_pp_edges
 *   checkpoint key layout                                   -> pf_set_weight (names are the
 *                                                                                  reference state_dict keys)
 * The reference has no FFI of its own: the seam is a Python method call, so these entry points are
 * what a ctypes binding added to the reference would bind.
 *
 * Conventions
 *   - every function returns 0 on success or a negative pf_status; pf_last_error(h) gives text;
 *     no exceptions cross the ABI;
 *   - the caller owns every tensor it passes (PyTorch allocations as raw device pointers + sizes);
 *     the library owns its packed weights and a workspace sized by pf_set_pocket_batch;
 *   - "dev" pointers are device memory of the current HIP device, "host" pointers host memory;
 *     all tensors are dense row-major fp32 (indices int32);
 *   - all work is ordered on the caller's stream: when the stream reaches the end of a call's work,
 *     every output of the call is complete.  Two calls also use streams of the handle, joined to the
 *     caller's stream by events -- pf_set_pocket_batch uploads its tables on a copy stream (the upload
 *     of the next batch runs under the kernels of the current one), pf_train_backward builds its work
 *     lists and sums finished gradient copies on a side stream.  No call synchronises the device
 *     except pf_create / pf_commit_weights / pf_set_pocket_batch when an allocation has to grow, and
 *     the pf_debug_* readers;
 *   - a handle is bound to one device and is not thread-safe (one handle per GPU / process).
 *   - there is NO CPU fallback: without a usable HIP device every compute call fails with
 *     PF_ERR_HIP.
 */
#ifndef PFDYN_H
#define PFDYN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_ABI_VERSION 1

typedef struct pf_handle pf_handle;
typedef void* pf_stream;           /* hipStream_t */

typedef enum pf_status {
    PF_OK = 0,
    PF_ERR_ARG = -1,           /* bad argument / unsupported configuration */
    PF_ERR_HIP = -2,           /* HIP runtime error (no device, OOM, launch failure) */
    PF_ERR_STATE = -3,         /* call order violated (weights not committed, no batch set ...) */
    PF_ERR_WEIGHT = -4,        /* unknown / missing / mis-shaped weight tensor */
    PF_ERR_EXCHANGE = -5       /* pf_sample_status: a workgroup hand-over inside a launch timed out; the run is invalid, repeat it */
} pf_status;

/* message_norm of GVPMultiEdgeConv (gvp.py:351,373-389) */
#define PF_NORM_MEAN 0         /* 'mean': mean reducer, divide by 1 */
#define PF_NORM_VALUE 1        /* number > 0: sum reducer, divide by message_norm_value */
#define PF_NORM_GRAPH 2        /* number == 0: sum reducer, divide by (edges into ntype)/(nodes of ntype)+1 per graph */

/* Mirrors PharmRecDynamicsGVP.__init__ (dynamics_gvp.py:96-97) + graph_cutoffs (configs/dev.yml:67-68). */
typedef struct pf_config {
    int32_t abi_version;        /* = PF_ABI_VERSION */
    int32_t pharm_nf;           /* n_pharm_scalars (6) */
    int32_t rec_nf;             /* n_prot_scalars  (11) */
    int32_t vector_size;        /* 16 or 32 (16 with n_hidden_scalars 128: the specialised kernels) */
    int32_t n_hidden_scalars;   /* 64..256, a multiple of 32; other than (128, 16): the width-generic family, inference only */
    int32_t n_convs;
    int32_t n_message_gvps;
    int32_t n_update_gvps;
    int32_t n_noise_gvps;
    int32_t message_norm_mode;  /* PF_NORM_* */
    float   message_norm_value;
    int32_t ff_k;               /* 0 = radius graph with cutoff_ff (max 200 neighbours) */
    int32_t pf_k;               /* 0 = radius with cutoff_pf (max 100 neighbours) */
    float   cutoff_pp, cutoff_pf, cutoff_fp, cutoff_ff;
    float   rbf_dmax;           /* 15 (gvp.py:350) */
    int32_t rbf_dim;            /* must be 16 */
} pf_config;

/* per-step scalars of sample_p_zs_given_zt (pharmacodiff.py:387-420), fp32, computed by the host */
typedef struct pf_step_coef {
    float t;                    /* (s+1)/T : the timestep fed to the dynamics            (:470) */
    float alpha_t_given_s;      /*                                                        (:156) */
    float var_terms;            /* sigma2_t_given_s / alpha_t_given_s / sigma_t           (:397) */
    float sigma;                /* sigma_t_given_s * sigma_s / sigma_t                    (:400) */
    float ep_zt;                /* endpoint param: alpha_t_given_s*sigma_s^2/sigma_t^2    (:414) */
    float ep_pred;              /* endpoint param: alpha_s*sigma2_t_given_s/sigma_t^2     (:414) */
} pf_step_coef;

/* per-step scalars of a pinned run (pf_denoise_step_pinned): the noise level of z_s, alpha(gamma(s/T)) and sigma(gamma(s/T))
 * (pharmacodiff.py:140-146), fp32, computed by the host */
typedef struct pf_pin_coef { float alpha_s; float sigma_s; } pf_pin_coef;

/* scalars of one resampling jump b -> a of a pinned run (pf_renoise_step): alpha_{a|b} and sigma_{a|b} of
 * sigma_and_alpha_t_given_s(gamma(a/T), gamma(b/T)) (pharmacodiff.py:148-160), fp32, computed by the host */
typedef struct pf_renoise_coef { float alpha_t_given_s; float sigma_t_given_s; } pf_renoise_coef;

const char* pf_version(void);
const char* pf_last_error(const pf_handle* h);     /* h may be NULL: last error of pf_create */

/* -- lifetime ------------------------------------------------------------------------------ */
int  pf_create(const pf_config* cfg, pf_handle** out);
void pf_destroy(pf_handle* h);

/* -- weights: one call per tensor of the reference state_dict under "dynamics." -------------
 * name: the reference key, e.g. "dynamics.noise_predictor.conv_layers.0.edge_message_fns.prot_pp_prot.0.Wh"
 * data: host fp32, row-major, shape[ndim].  Zero-size tensors (dropout dummy_param) and
 * "gamma.gamma" are accepted and ignored.  pf_commit_weights fails if any tensor is missing. */
int pf_set_weight(pf_handle* h, const char* name, const float* host_data, int32_t ndim, const int64_t* shape);
int pf_commit_weights(pf_handle* h);

/* -- static per-batch data (the DGL-free batch container) -----------------------------------
 * B graphs; graph g owns prot atoms [prot_ptr[g], prot_ptr[g+1]) and pharmacophore centers
 * [pharm_ptr[g], pharm_ptr[g+1]).  pp edges (static prot->prot, batch-local prot ids) may be in
 * any order (destination-sorted lists inside their graphs take a vectorised pass; anything else a scalar one that also
 * reports what is wrong).  prot_x / prot_h are copied into the handle's memory.  Asynchronous: the host tables are built in
 * pinned memory owned by the handle and uploaded with one copy (on the handle's copy stream, ordered before everything the
 * caller enqueues on `stream` afterwards); the host arrays may be freed on return.  The call synchronises the device only
 * when the workspace or a table buffer has to grow. */
int pf_set_pocket_batch(pf_handle* h, int32_t B, const int32_t* host_prot_ptr, const int32_t* host_pharm_ptr,
                        const float* dev_prot_x, const float* dev_prot_h,
                        int64_t n_pp, const int32_t* host_pp_src, const int32_t* host_pp_dst, pf_stream stream);

/* The same bind for callers whose pocket data lives on the HOST (the sampling drivers batch pockets on the host):
 * prot_x [Np,3] / prot_h [Np,rec_nf] are host fp32 arrays; they travel in the same single staged upload as the index
 * tables and the one-hot check runs on the host copy, so the call never waits for the device. */
int pf_set_pocket_batch_host(pf_handle* h, int32_t B, const int32_t* host_prot_ptr, const int32_t* host_pharm_ptr,
                             const float* host_prot_x, const float* host_prot_h,
                             int64_t n_pp, const int32_t* host_pp_src, const int32_t* host_pp_dst, pf_stream stream);

/* Optional, BEFORE the next pf_set_pocket_batch / _host call: host_rep[g] = index of the graph that represents graph g's
 * pocket (host_rep[r] == r for a representative).  The caller claims that graph g is a COPY of graph host_rep[g] -- same
 * atoms, features, coordinates and pp edges -- which is how every sampling batch of the reference is built
 * (copy_graph, utils/unorganized_utils.py:28-81; pharmacodiff.py:541-545; generate_pharmacophores.py:329-333).  The bind
 * verifies the claim (everything it can see on the host) and fails with PF_ERR_ARG if it does not hold.  Effect: during
 * sampling, copies at the same timestep share conv layer 0's protein->protein messages (computed once per pocket
 * instead of once per copy, gvp.py:545-549 being a pure function of pocket geometry, element types and t there);
 * outputs are the same up to fp32 summation order.  The groups apply to one bind only -- the next bind call consumes the
 * claim whether it succeeds or is rejected (argument checks included).  What "verifies" covers: ptr arrays and pp edges
 * always (they are host arrays), coordinates and features on the host for pf_set_pocket_batch_host.  With pf_set_pocket_batch
 * (DEVICE coordinates / features) the rows are compared on the device by a small launch of the bind (bit patterns, every atom
 * against the same atom of its representative); the verdict comes back through pinned memory and the first call that would
 * share messages (pf_dynamics_forward / pf_denoise_step / pf_sample of that batch) reads it and fails with PF_ERR_ARG if the
 * claim is false -- nothing is ever computed on a false claim. */
int pf_set_pocket_groups(pf_handle* h, int32_t B, const int32_t* host_rep);

/* Optional, right after pf_set_pocket_batch: the caller states whether every row of prot_h is an element one-hot
 * (what the reference's dataset / CLI always produce: protein_pharm_dataset.py:129, generate_pharmacophores.py:105-118).
 * pf_set_pocket_batch checks this on the device and the first inference call that wants the answer waits for it; a caller
 * that already knows (it built the rows, or checked them on the host) says so here and no call ever waits: the whole
 * bind is then asynchronous on `stream`.  Declaring 1 for rows that are not one-hots gives wrong results. */
int pf_declare_onehot_features(pf_handle* h, int32_t is_onehot);

/* radius_graph(prot, r=cutoff_pp, max_num_neighbors) per graph on the device; results on the host.
 * Call with host_src == NULL to get the edge count (return value >= 0), then again with buffers. */
int64_t pf_build_pp_edges(pf_handle* h, int32_t B, const int32_t* host_prot_ptr, const float* dev_prot_x,
                          int32_t max_num_neighbors, int32_t* host_src, int32_t* host_dst, int64_t capacity,
                          pf_stream stream);

/* -- the boundary function: (eps_h, eps_x) = dynamics(g, t) ---------------------------------
 * dev_prot_x may be NULL (use the coordinates currently held by the handle).
 * Pure with respect to the handle's sampling state. */
int pf_dynamics_forward(pf_handle* h, const float* dev_prot_x, const float* dev_pharm_x, const float* dev_pharm_h,
                        const float* dev_t /*[B]*/, float* dev_eps_h /*[Nf,pharm_nf]*/, float* dev_eps_x /*[Nf,3]*/,
                        pf_stream stream);

/* -- sampling state machine (sample_given_receptor, pharmacodiff.py:433-488) ----------------
 * begin : prot -= init_pharm_com[graph] (NULL: protein COM); x_t,h_t := init noise
 * step  : one sample_p_zs_given_zt with injected noise (x columns before h columns)
 * end   : remove protein COM, add initial protein COM, multiply h by feat_norm_constant */
int pf_sample_begin(pf_handle* h, const float* dev_init_pharm_com /*[B,3] or NULL*/,
                    const float* dev_noise0 /*[Nf,3+pharm_nf]*/, pf_stream stream);
int pf_denoise_step(pf_handle* h, const pf_step_coef* coef, const float* dev_noise /*[Nf,3+pharm_nf]*/,
                    int32_t endpoint_param_coord, int32_t endpoint_param_feat, pf_stream stream);
int pf_sample_end(pf_handle* h, float feat_norm_constant, float* dev_x0 /*[Nf,3]*/, float* dev_h0 /*[Nf,pharm_nf]*/,
                  pf_stream stream);
/* Validity of the sampling runs that ended (pf_sample_end / pf_sample) since the last call.  For small batches a step's last
 * launch hands the noise prediction from its node + head workgroups to its update + build workgroups through polled exchange
 * words (k_rg_node_hs_build); the poll is bounded, so a hand-over that never arrives (never observed: producers do not wait and
 * the whole grid is resident) ends the launch on zeros instead of hanging the device -- and the run is INVALID.  The count of
 * such time-outs is copied to pinned host memory behind the results of pf_sample_end, on the caller's stream: call this AFTER
 * waiting for x_0 / h_0 (stream or event synchronisation -- the call itself touches no device and never blocks) and BEFORE
 * using them.  Returns PF_OK, or PF_ERR_EXCHANGE with *n_timeouts (may be NULL) = the new time-outs; the handle then runs the
 * separate launches (as with PFDYN_HS_BUILD=0), so repeating the run on it is safe.  A caller that never asks is told by the
 * next pf_sample_begin on the handle, which fails with the same code.  The reference has nothing to correspond: its
 * sample_given_receptor (pharmacodiff.py:433-514) is host-sequenced. */
int pf_sample_status(pf_handle* h, int32_t* n_timeouts);
/* current frame in the caller's frame of reference (get_pos_feat_for_visual, pharmacodiff.py:360-378) */
int pf_sample_frame(pf_handle* h, float feat_norm_constant, float* dev_x /*[Nf,3]*/, float* dev_h /*[Nf,pharm_nf]*/,
                    pf_stream stream);
/* Optional, after pf_set_pocket_batch and before a loop of pf_denoise_step calls: the timesteps (pf_step_coef::t) the loop will visit.  The first
 * conv layer's protein-side messages depend on t only through one encoder output per element type
 * (dynamics_gvp.py:107-117 feeding gvp.py:545-549); their tables are computed here in one launch per 64 timesteps
 * instead of one small launch in front of every step.  pf_sample does this itself; results never depend on it. */
int pf_prepare_timesteps(pf_handle* h, const float* host_t, int32_t n, pf_stream stream);
/* whole loop: begin + n_steps x step + end, all enqueued on `stream` without host synchronisation.
 * host_coef[i] is the i-th iteration's coefficients (s = T-1-i); dev_noise is [n_steps+1, Nf, 3+pharm_nf].
 * dev_traj_x / dev_traj_h (optional) receive n_steps+1 frames. */
int pf_sample(pf_handle* h, int32_t n_steps, const pf_step_coef* host_coef, const float* dev_noise,
              const float* dev_init_pharm_com, int32_t endpoint_param_coord, int32_t endpoint_param_feat,
              float feat_norm_constant, float* dev_x0, float* dev_h0, float* dev_traj_x, float* dev_traj_h,
              pf_stream stream);

/* -- pinned centers: complete a pharmacophore around given points (replacement conditioning; no reference counterpart) ----------
 * Every center carries a 2-bit flag: bit 0 = its position is given, bit 1 = its feature row is given (0 = free, 3 = both).
 * dev_pin_x are positions in the CALLER's frame (the frame of the pocket coordinates bound with pf_set_pocket_batch);
 * dev_pin_h are the raw rows the caller wants back (normally type one-hots; the run divides them by feat_norm_constant).  Rows of
 * free centers are ignored.  A pinned run is pf_sample with one change per step: iteration i handles s = T-1-i, and after the
 * usual p(z_s | z_t) values, for every graph g and center f of it
 *     c_cur[g] = mean of the graph's current protein rows (before this step's shift)
 *     D[g]     = c_init[g] - c_cur[g]        c_init = mean of the original protein coordinates; caller's frame = sampler frame + D
 *     bit 0:  x_s[f] = alpha_s * (pin_x[f] - D[g]) + sigma_s * noise_x[f]
 *     bit 1:  h_s[f] = alpha_s * (pin_h[f] / feat_norm_constant) + sigma_s * noise_h[f]
 * with this step's own noise draw of the center (one rounding per operation); then the COM of ALL centers of the graph is removed
 * from centers and protein as in pf_denoise_step.  The initial draw is not touched.  pf_sample_end (and the last trajectory
 * frame of pf_sample_pinned) returns the given values bit for bit; earlier frames show the noised state.
 * pf_sample_begin_pinned = pf_sample_begin + the handle's own copy of the three pin arrays (stream-ordered; the allocation is kept
 * and reused, and grows -- with a stream synchronisation -- only when a batch has more centers).  The run is pinned until the next
 * pf_sample_begin / pf_sample_begin_pinned / pf_set_pocket_batch: inside it pf_denoise_step returns PF_ERR_STATE, and so does
 * pf_denoise_step_pinned outside it.  A pinned step never takes the tail or merged launches of pf_denoise_step: its dynamics call
 * is followed by one launch of its own (k_step_build<MovePinned>: the update above + the generic edge build; k_step_update<MovePinned> for the
 * width-generic family), so it costs one launch per step more than the default path, and pf_debug_kernel_family(h, n_convs)
 * reports 0 after it.  Unpinned runs are not affected.
 * pf_sample_pinned: pf_sample's arguments + host_pin_coef[n_steps] (entry i: s = T-1-i) + the three pin arrays. */
int pf_sample_begin_pinned(pf_handle* h, const float* dev_init_pharm_com /*[B,3] or NULL*/, const float* dev_noise0 /*[Nf,3+pharm_nf]*/,
                           const int32_t* dev_pin_flags /*[Nf], 0..3*/, const float* dev_pin_x /*[Nf,3]*/,
                           const float* dev_pin_h /*[Nf,pharm_nf]*/, float feat_norm_constant, pf_stream stream);
int pf_denoise_step_pinned(pf_handle* h, const pf_step_coef* coef, const pf_pin_coef* pin_coef, const float* dev_noise /*[Nf,3+pharm_nf]*/,
                           int32_t endpoint_param_coord, int32_t endpoint_param_feat, pf_stream stream);
int pf_sample_pinned(pf_handle* h, int32_t n_steps, const pf_step_coef* host_coef, const pf_pin_coef* host_pin_coef,
                     const float* dev_noise, const float* dev_init_pharm_com, const int32_t* dev_pin_flags, const float* dev_pin_x,
                     const float* dev_pin_h, int32_t endpoint_param_coord, int32_t endpoint_param_feat, float feat_norm_constant,
                     float* dev_x0, float* dev_h0, float* dev_traj_x, float* dev_traj_h, pf_stream stream);

/* -- pinned runs with resampling jumps (RePaint, Lugmayr et al. 2022; no reference counterpart) --------------------------------
 * In a pinned run the given centers are drawn at every step independently of what the free centers just became.  Resampling lets
 * the free centers react: after a stretch of reverse steps the whole state is diffused forward again to the stretch's upper noise
 * level and the stretch is denoised again.  Let T be the number of timesteps, `jump` j >= 1 and `resamples` r >= 1.
 * Levels run T -> 0.  Segment tops are a_0 = T and a_(k+1) = max(a_k - j, 0), until 0.  A segment is (a, b) with a > b; its length
 * is j, except possibly the last one.  D(s) is the pinned denoise step with coefficient index s (t = s+1 -> s,
 * pf_denoise_step_pinned); R(b->a) is the re-noise op (pf_renoise_step).  The plan of a run is, segment after segment from the top:
 *     D(a-1) ... D(b),   then (r - 1) times:  R(b->a), D(a-1) ... D(b)
 * The last segment, which ends at level 0, is resampled like the others.  r = 1 gives exactly D(T-1) ... D(0).
 * Example, T = 7, j = 3, r = 2:   D6 D5 D4 R(4->7) D6 D5 D4 | D3 D2 D1 R(1->4) D3 D2 D1 | D0 R(0->1) D0   -- 17 ops.
 * R(b->a) acts on every graph g and every center f of it, pinned and free centers alike, coordinates and feature rows alike:
 *     z_a[f] = alpha_{a|b} * z_b[f] + sigma_{a|b} * noise[f]                     (one rounding per operation, no contraction)
 * then the COM of all centers of the graph is removed from centers and protein (the reduction order of pf_denoise_step's update),
 * and the dynamic edges of the next dynamics call are built on the new coordinates.  alpha_{a|b} and sigma_{a|b} come from
 * sigma_and_alpha_t_given_s(gamma(a/T), gamma(b/T)), in fp32 on the host.  One forward jump over the whole segment is used, not j
 * single steps: it has the same distribution and costs one launch.  No frame offset D[g] is needed, because nothing of the
 * caller's frame enters.  A pinned center needs no special case: at level b it holds the given value noised to level b, the forward
 * move gives it the right marginal at level a, and the following D op replaces it anyway.
 * pf_renoise_step is valid only inside a pinned run (outside one: PF_ERR_STATE; a caller who wants resampling without pins begins a
 * pinned run with all flags zero); a null argument is PF_ERR_ARG.  It makes no dynamics call: one launch (k_step_build<MoveRenoise>: the
 * move + the generic edge build; k_step_update<MoveRenoise> for the width-generic family and every configuration whose next dynamics call
 * builds its own edges), on the caller's stream, no host synchronisation.  pf_debug_kernel_family(h, n_convs) reports 0 after it.
 * pf_sample_pinned_resampled: pf_sample_pinned's arguments with n_ops in place of n_steps, plus host_op[n_ops] (0 denoise, 1 renoise;
 * anything else: PF_ERR_ARG before anything is enqueued) and host_renoise[n_ops].  host_coef[i] and host_pin_coef[i] are read for op
 * kind 0, host_renoise[i] for kind 1; the other entries are ignored.  dev_noise is [n_ops + 1, Nf, 3 + pharm_nf]: row 0 is the
 * initial draw and row 1 + i belongs to op i, whatever its kind.  A trajectory has n_ops + 1 frames; the last frame and x_0 / h_0
 * carry the given values bit for bit.  Unpinned runs, and pinned runs without resampling, are not affected. */
int pf_renoise_step(pf_handle* h, const pf_renoise_coef* coef, const float* dev_noise /*[Nf,3+pharm_nf]*/, pf_stream stream);
int pf_sample_pinned_resampled(pf_handle* h, int32_t n_ops, const int32_t* host_op /*[n_ops]: 0 denoise, 1 renoise*/,
                               const pf_step_coef* host_coef, const pf_pin_coef* host_pin_coef, const pf_renoise_coef* host_renoise /*[n_ops]*/,
                               const float* dev_noise, const float* dev_init_pharm_com, const int32_t* dev_pin_flags, const float* dev_pin_x,
                               const float* dev_pin_h, int32_t endpoint_param_coord, int32_t endpoint_param_feat, float feat_norm_constant,
                               float* dev_x0, float* dev_h0, float* dev_traj_x, float* dev_traj_h, pf_stream stream);

/* -- guided sampling: restraint energies steer the centers (reconstruction guidance; no reference counterpart) ------------------
 * A guided run is a pinned run (pf_sample_begin_pinned's state; the flags may all be zero) plus a set of restraints per graph.
 * A restraint is (kind, center, p[3], r, w): kind 0 attract / 1 repel; center a local center index in [0, nf_g) or -1 for every
 * center of the graph; p in the CALLER's frame, as pin_x is; r >= 0, w >= 0.  For a center f it applies to, with y_f the predicted
 * clean center in the caller's frame and rho = |y_f - p| (plain sqrtf):
 *     attract:  E = w * max(0, rho - r)^2      dE/dy_f =  2 w max(0, rho - r) (y_f - p) / rho
 *     repel  :  E = w * max(0, r - rho)^2      dE/dy_f = -2 w max(0, r - rho) (y_f - p) / rho          rho == 0: the gradient is 0
 * (both C1).  Step i handles s = T-1-i, with D[g] as in a pinned run (caller's frame = sampler frame + D, taken before this step's
 * shift) and alpha_t, sigma_t of level t = s+1 (pf_guide_coef):
 *     eps        = dynamics(z_t, t)                      the width-generic training forward, dropout 0 (it keeps what the VJP reads)
 *     x0_hat[f]  = (x_t[f] - sigma_t eps_x[f]) / alpha_t   noise parameterisation;   = eps_x[f]   endpoint_param_coord
 *     y_f        = x0_hat[f] + D[g]
 *     g0[f]      = sum over the graph's restraints j that apply to f, j ascending, of dE_j/dy_f          (fp32, this order)
 *     E[g]       = sum over f ascending, j ascending, of E_j(y_f)
 *     J(u)       = d(sum eps_x . u)/d x_t: the VJP of the dynamics (pf_dynamics_input_vjp's g_pharm_x with g_eps_h = 0)
 *     grad[f]    = g0[f] / alpha_t - (sigma_t / alpha_t) J(g0)[f]   noise parameterisation;   = J(g0)[f]   endpoint_param_coord
 *     shift[f]   = guide_scale * coef.sigma^2 * grad[f]   (posterior mean + scale * posterior variance * grad log p, log p = -E)
 *     if guide_clip > 0 and |shift[f]| > guide_clip:  shift[f] *= guide_clip / |shift[f]|
 *     x_s[f]     = (the usual p(z_s | z_t) value) - shift[f]
 * then the pin selects (a position-pinned center ignores its shift) and the COM removal, exactly as in a pinned step.  One rounding
 * per operation.  Features are not guided (h_s is the plain update).  D[g] is a constant for d(y)/d(x_t), and the edge sets carry
 * no gradient (pf_train_backward_inputs).  A graph without restraints has g0 = 0 and, in the noise parameterisation, shift = 0
 * exactly.
 * The handle must be on PF_TRAIN_FAMILY_WIDE (otherwise PF_ERR_STATE: call pf_train_set_family first) -- or, a 128 / 16 handle, on
 * PF_TRAIN_FAMILY_TUNED with pf_train_set_input_grads(h, 1): the step's training forward and inputs-only backward then run on the
 * tuned kernels (fp32; PF_ERR_ARG with PF_TRAIN_BF16 selected).  The run records the family and the switch it began on, and a step
 * after either changed is PF_ERR_STATE.  A 128 / 16 handle's unguided
 * runs stay on the tuned kernels.  pf_sample_begin_guided takes pf_sample_begin_pinned's arguments and HOST arrays restr_ptr[B+1]
 * (graph g owns restraints [restr_ptr[g], restr_ptr[g+1])), restr_kind[n], restr_center[n], restr_p[n][3], restr_r[n], restr_w[n].
 * Everything is validated on the host before anything is enqueued (kind, center range, finite p, r / w / scale / clip >= 0, at most
 * 256 restraints per graph; csrc/pf_restr.h): a failure is PF_ERR_ARG and leaves the handle as it was.  The restraints travel through a pinned
 * staging buffer into one allocation of the handle, kept and grown like the pin arrays; the host arrays may be freed on return.
 * A guided run ends at the next begin of any kind or the next bind.  Inside it pf_denoise_step, pf_denoise_step_pinned and
 * pf_renoise_step return PF_ERR_STATE (guidance with resampling jumps is not supported), and so does pf_denoise_step_guided outside
 * it.  A guided step costs the training forward, two small launches and the inputs-only backward, all on the caller's stream
 * without host synchronisation; pf_debug_kernel_family(h, n_convs) reports 0 after it.
 * pf_sample_guided: pf_sample_pinned's arguments + host_guide_coef[n_steps] (entry i: s = T-1-i), the restraint arrays, scale, clip,
 * and dev_energy [n_steps, B] (optional): E[g] as step i computed it. */
typedef struct pf_guide_coef { float alpha_t; float sigma_t; } pf_guide_coef;      /* alpha / sigma(gamma((s+1)/T)), fp32, computed by the host */
int pf_sample_begin_guided(pf_handle* h, const float* dev_init_pharm_com /*[B,3] or NULL*/, const float* dev_noise0 /*[Nf,3+pharm_nf]*/,
                           const int32_t* dev_pin_flags /*[Nf], 0..3*/, const float* dev_pin_x /*[Nf,3]*/, const float* dev_pin_h /*[Nf,pharm_nf]*/,
                           float feat_norm_constant, const int32_t* host_restr_ptr /*[B+1]*/, const int32_t* host_restr_kind /*[n]*/,
                           const int32_t* host_restr_center /*[n]*/, const float* host_restr_p /*[n,3]*/, const float* host_restr_r /*[n]*/,
                           const float* host_restr_w /*[n]*/, float guide_scale, float guide_clip, pf_stream stream);
int pf_denoise_step_guided(pf_handle* h, const pf_step_coef* coef, const pf_pin_coef* pin_coef, const pf_guide_coef* guide_coef,
                           const float* dev_noise /*[Nf,3+pharm_nf]*/, int32_t endpoint_param_coord, int32_t endpoint_param_feat, pf_stream stream);
int pf_sample_guided(pf_handle* h, int32_t n_steps, const pf_step_coef* host_coef, const pf_pin_coef* host_pin_coef,
                     const pf_guide_coef* host_guide_coef, const float* dev_noise, const float* dev_init_pharm_com,
                     const int32_t* dev_pin_flags, const float* dev_pin_x, const float* dev_pin_h, int32_t endpoint_param_coord,
                     int32_t endpoint_param_feat, float feat_norm_constant, const int32_t* host_restr_ptr, const int32_t* host_restr_kind,
                     const int32_t* host_restr_center, const float* host_restr_p, const float* host_restr_r, const float* host_restr_w,
                     float guide_scale, float guide_clip, float* dev_x0, float* dev_h0, float* dev_traj_x, float* dev_traj_h,
                     float* dev_energy /*[n_steps,B] or NULL*/, pf_stream stream);
/* tests: the last guided step's vectors, each nullable -- g0, grad, shift [Nf,3] (a position-pinned center's rows are what it
 * ignored) and E [B]; PF_ERR_STATE when no guided step has run on this batch */
int pf_debug_last_guidance(pf_handle* h, float* dev_g0, float* dev_grad, float* dev_shift, float* dev_energy, pf_stream stream);

/* -- pocket field: clash avoidance and complementarity energies next to a guided run's restraints (no reference counterpart) ------
 * A guided run may carry a pocket field: two energies that come from the pocket itself and are added to the restraints' (there may
 * be none of those) in the formulas above -- x0_hat, y_f = x0_hat[f] + D[g], g0, E[g], grad, shift.  Every element is optional.
 * Clash.  HOST radii atom_r[Np_tot] >= 0 (0: the atom is inert) and a weight w_clash >= 0.  With a_i the CURRENT protein row of
 * the sampler's frame and rho = |x0_hat[f] - a_i| (the sampler's frame: x0_hat and a_i are both there, and the distance is the one
 * of the caller's frame), for every center f and every atom i of its graph:
 *     E       += w_clash * max(0, atom_r[i] - rho)^2
 *     dE/dy_f  = -2 w_clash max(0, atom_r[i] - rho) (x0_hat[f] - a_i) / rho,   0 when rho == 0
 * Complementarity.  Per graph receptor features (q_j, u_j) in the caller's frame: HOST ph_ptr[B+1], ph_x[n][3], ph_type[n] with
 * 0 <= ph_type < pharm_nf; a HOST match table M[pharm_nf][pharm_nf] (0 / 1: a center of type t is matched by a receptor feature
 * of type u) and distances d[pharm_nf] >= 0; w_comp >= 0, kappa > 0, type_sharpness >= 0.  Center f has type weights
 *     p_f = softmax_t(type_sharpness * h0_hat[f]),  h0_hat = (h_t - sigma_t eps_h) / alpha_t, or eps_h under endpoint_param_feat
 * which are constants of the differentiation (the VJP's g_eps_h stays zero) unless type guidance's comp_types is on, below.  For every type t whose set
 * S_t = {j : M[t][u_j]} is non-empty in the graph, with rho_j = |y_f - q_j|:
 *     rho~ = -(1/kappa) log sum_{j in S_t} exp(-kappa rho_j)     (evaluated with the largest exponent subtracted)
 *     s_j  = the softmax weights of that sum,  m = max(0, rho~ - d[t])
 *     E       += w_comp p_ft m^2
 *     dE/dy_f += w_comp p_ft 2 m sum_j s_j (y_f - q_j) / rho_j   (a term with rho_j == 0 contributes 0)
 * rho~ <= min_j rho_j: a center with a matching feature of type-t partners within d[t] -- what the validity metric counts as
 * matched -- pays nothing for t.  The converse holds up to log|S_t| / kappa: a center that pays nothing for t has its nearest
 * partner within d[t] + log|S_t| / kappa.  Both energies are C1.
 * Totals.  g0[f] = (restraints' sum + clash gradient) + complementarity gradient; E[g] likewise, and dev_energy's rows hold the
 * total.  The VJP, shift, clip, pin selects and COM removal are unchanged.  A graph without features, and atoms of radius 0,
 * contribute exact zeros.  The sums' order is fixed: the same bits on every run.
 * Arming.  pf_guide_field_next comes after a bind and arms the NEXT pf_sample_begin_guided (also the one inside pf_sample_guided),
 * which consumes it, accepted or not; the field ends with that run.  atom_r NULL: no clash term; ph_ptr NULL: no complementarity
 * term (the arrays behind it are then not read).  It validates on the host before anything is touched -- finite, non-negative
 * radii, weights and distances; kappa > 0; types in range; a table of 0 / 1; ph_ptr[0] == 0, monotone, at most 4096 features per
 * graph: a failure is PF_ERR_ARG with a message and leaves the handle as it was (a field armed before stays armed).  The arrays are
 * copied into a handle-owned pinned buffer before the call returns.  The begin of any other run kind while a field is armed
 * returns PF_ERR_STATE and drops the arming; so does a bind (silently).  A run in progress is not touched by any of this.
 * pf_debug_last_field: the three components of the last guided step per graph, [B][3]: restraints, clash, complementarity
 * (their sum in that order is E[g]); PF_ERR_STATE when the last guided step on this batch had no field. */
int pf_guide_field_next(pf_handle* h, const float* host_atom_r /*[Np_tot] or NULL*/, float w_clash, const int32_t* host_ph_ptr /*[B+1] or NULL*/,
                        const float* host_ph_x /*[n,3]*/, const int32_t* host_ph_type /*[n]*/, const int32_t* host_match /*[pharm_nf,pharm_nf]*/,
                        const float* host_dist /*[pharm_nf]*/, float w_comp, float kappa, float type_sharpness);
int pf_debug_last_field(pf_handle* h, float* dev_E3 /*[B,3]*/, pf_stream stream);

/* -- type guidance: a guided run also steers the centers' feature rows (no reference counterpart) --------------------------------
 * The names are those above: x0_hat, y_f = x0_hat[f] + D[g], alpha_t, sigma_t, coef.sigma.
 * Predicted clean features.  h0_hat[f] = (h_t[f] - sigma_t eps_h[f]) / alpha_t, or eps_h[f] under endpoint_param_feat;
 * p_f = softmax_k(s * h0_hat[f][k]) with s = type_sharpness, the maximum subtracted first.
 * Type restraint (center, type c, p[3], r, w): center a local index or -1 for every center of the graph, 0 <= c < pharm_nf, p in
 * the caller's frame, r, w >= 0, at most 256 per graph.  Window: omega = 1 when r == 0 (no spatial condition), otherwise
 * q = max(0, 1 - rho^2 / r^2), omega = q^2, rho^2 = |y_f - p|^2 (no square root; C1 and compact).
 *     CE = log(sum_k exp(s h0_hat[k] - max)) + max - s h0_hat[c]         (= -log p_fc)
 *     E  = w omega CE
 *     dE/dh0_hat[k] = w omega s (p_fk - [k == c])
 *     dE/dy_f       = w CE (2 q) (-2 (y_f - p) / r^2),   exactly zero when r == 0 or q == 0
 * Inside the sphere a center either takes type c or is pushed out; with an attract restraint on the same sphere this reads "a
 * center of type c within r of p".
 * Complementarity with a type gradient (comp_types, and a pocket field with features and w_comp > 0).  m_t is the pocket field's
 * hinge for a type whose set S_t is non-empty in the graph and m_t = unmatched (>= 0, default 0) for a type whose set is empty:
 *     dE/dh0_hat[f][k] = w_comp s p_fk (m_k^2 - sum_t p_ft m_t^2)
 * E_comp and its coordinate gradient keep their bits; w_comp sum_f sum_{t: S_t empty} p_ft unmatched^2 is counted under the type
 * energy, not in pf_debug_last_field's three components.  comp_types without such a field is accepted and inert.
 * Totals.  g0_h[f] = the restraints' term (j ascending) + the complementarity term; E_type[g] = type restraints + unmatched term;
 * E[g] = (((E_restr + E_clash) + E_comp) + E_type); g0[f] gains the windows' coordinate term behind the field's.
 * Through the network.  phi_x = -sigma_t / alpha_t (noise parameterisation) or 1 (endpoint_param_coord); phi_h likewise from
 * endpoint_param_feat.  The VJP runs once with g_eps_x = g0 and g_eps_h = (phi_h / phi_x) g0_h and returns J_x, J_h:
 *     grad_x     = [g0 / alpha_t, noise only] + phi_x J_x           (the guided step's expression)
 *     grad_h[f]  = [g0_h[f] / alpha_t, noise feat only] + phi_x J_h[f]
 *     shift_h[f] = feat_scale * coef.sigma^2 * grad_h[f], clipped to Euclidean norm feat_clip over the row when feat_clip > 0
 *     h_s[f]     = (the usual value) - shift_h[f]   unless the center's type is pinned (flag & 2)
 * One rounding per operation.  J_h carries the coordinate energies too: with feat_scale > 0 the feature rows follow every energy
 * of the run; feat_scale == 0 leaves them where the run without the arming puts them, bit for bit.
 * Arming.  pf_guide_types_next comes after a bind and arms the NEXT pf_sample_begin_guided (also the one inside pf_sample_guided),
 * which consumes it, accepted or not; it ends with that run.  host_ptr NULL: no type restraint.  Validation on the host before
 * anything is touched -- ranges against the bound pharm_ptr, finite values, non-negative r, w, scale, clip, sharpness and
 * unmatched, the per-graph cap: a failure is PF_ERR_ARG and leaves the handle as it was.  When a pocket field is armed too, both
 * type_sharpness values must agree or the begin returns PF_ERR_ARG.  The begin of any other run kind while it is armed returns
 * PF_ERR_STATE and drops the arming; so does a bind (silently).  Without type restraints no k_guide_types launch is made, without
 * comp_types the pocket field's launch is the one it was; a guided run without the arming executes exactly the launches it did.
 * pf_debug_last_type_guidance: the last guided step's g0_h, grad_h, shift_h [Nf,pharm_nf] (a type-pinned center's rows are what
 * it ignored) and E_type [B], each nullable; PF_ERR_STATE when the last guided step on this batch ran without the arming. */
int pf_guide_types_next(pf_handle* h, const int32_t* host_ptr /*[B+1] or NULL*/, const int32_t* host_center /*[n]*/,
                        const int32_t* host_type /*[n]*/, const float* host_p /*[n,3]*/, const float* host_r /*[n]*/,
                        const float* host_w /*[n]*/, float feat_scale, float feat_clip, float type_sharpness, int32_t comp_types,
                        float unmatched);
int pf_debug_last_type_guidance(pf_handle* h, float* dev_g0_h, float* dev_grad_h, float* dev_shift_h, float* dev_E_type, pf_stream stream);

/* -- pair guidance: distance restraints between two centers of one sample (no reference counterpart) ------------------------------
 * Every energy above is a sum over single centers; a pair restraint relates two centers of the same graph: "centers 0 and 3 five
 * to seven angstroms apart", "no two centers closer than 3".  The names are those above: x0_hat, D[g], alpha_t, sigma_t.
 * Pair restraint of graph g: (i, j, lo, hi, w).  i, j local center indices in [0, nf_g) or -1 for "every center"; with both given,
 * i != j; 0 <= lo <= hi, lo finite, hi finite or +inf (no upper bound); w >= 0 and finite; at most 256 per graph
 * (PF_PAIRS_MAX_PER_GRAPH).  The unordered pairs {a, b}, a != b, it covers: both given, {i, j}; one wildcard, {i, b} for every
 * b != i; both wildcards, every a < b.  A graph with fewer than two centers has no pairs and contributes exact zeros.
 * The point of center f.  y_f = x0_hat[f] + D[g] for a free center; y_f = pin_x[f] for a position-pinned one (flag bit 0): the
 * given position, in the caller's frame, a constant -- what the network predicts for a pinned center is not where it will be.
 * For a covered pair, d = y_a - y_b, rho = sqrtf((dx*dx + dy*dy) + dz*dz), one rounding per operation:
 *     m_lo = max(0, lo - rho)      m_hi = max(0, rho - hi)      (hi = +inf: m_hi = 0)
 *     E       = w (m_lo^2 + m_hi^2)
 *     dE/dy_a = ((2 w) (m_hi - m_lo) / rho) d,   dE/dy_b = -dE/dy_a,   both 0 when rho == 0
 * A position-pinned center receives no pair gradient: its g_pair row is exactly zero; the pair still counts in E and its free
 * partner still gets its half of the gradient.
 * Totals and their order.  For center f the terms of its covered partners are taken restraints ascending and, within a restraint,
 * partners b ascending, in four partial sums by (b & 3) that meet as (s0 + s1) + (s2 + s3): that is g_pair[f]; e_f is the same
 * sum of E over the pairs with f < b; E_pair[g] = sum_f e_f, f ascending, summed by one thread.  The pair launch (k_guide_pairs)
 * is the last one in front of the VJP, behind k_guide_grad, the pocket field's launch and k_guide_types:
 *     g0[f] += g_pair[f]          E[g] = ((((E_restr + E_clash) + E_comp) + E_type) + E_pair)
 * dev_energy's row is rewritten with the total; pf_debug_last_field's three components and E_type keep their meaning and their
 * bits.  The VJP, shift, clip, pin selects and COM removal are unchanged; the pair energies do not depend on the features.
 * Arming: pf_guide_types_next's rules.  pf_guide_pairs_next comes after a bind and arms the NEXT pf_sample_begin_guided (also the
 * one inside pf_sample_guided), which consumes it, accepted or not; it ends with that run.  HOST arrays ptr[B+1] (graph g owns
 * restraints [ptr[g], ptr[g+1])), i, j, lo, hi, w [n], copied before the call returns.  Validation on the host before anything is
 * touched (csrc/pf_pairs.h): a failure is PF_ERR_ARG with a message and leaves the handle as it was -- an earlier arming stays
 * armed.  The begin of any other run kind while it is armed returns PF_ERR_STATE and drops the arming; a bind drops it silently;
 * a run in progress is untouched.  host_ptr NULL, or no restraint in any graph: accepted and inert -- no pair launch is made and
 * the guided run executes exactly the launches it did.  The block goes through the guided begin's staged upload into an
 * allocation of the handle, kept and grown like the pin arrays.
 * pf_debug_last_pairs: the last guided step's g_pair [Nf,3] and E_pair [B], each nullable; PF_ERR_STATE when the last guided step
 * on this batch made no pair launch. */
#define PF_PAIRS_MAX_PER_GRAPH 256
int pf_guide_pairs_next(pf_handle* h, const int32_t* host_ptr /*[B+1] or NULL*/, const int32_t* host_i /*[n]*/, const int32_t* host_j /*[n]*/,
                        const float* host_lo /*[n]*/, const float* host_hi /*[n]*/, const float* host_w /*[n]*/);
int pf_debug_last_pairs(pf_handle* h, float* dev_g_pair /*[Nf,3]*/, float* dev_E_pair /*[B]*/, pf_stream stream);

/* -- sample sets: what the samples of one pocket agree on (no reference counterpart) ---------------------------------
 * A set is the S samples of one pocket, 1 <= S <= 1024; sample a has n_a centers, 1 <= n_a <= 64, positions x_ai in the caller's
 * frame and integer types t_ai in [0, pharm_nf).  All samples of a pocket live in the pocket's frame: nothing is aligned, and sets
 * of different pockets do not compare.  Type identity is exact.  With sigma > 0, tolerance >= 0 and threshold in [0, 1]:
 *   overlap      O(a,b) = sum_i sum_j [t_ai == t_bj] exp(-|x_ai - x_bj|^2 / (2 sigma^2))
 *   similarity   sim(a,b) = O(a,b) / (O(a,a) + O(b,b) - O(a,b)); the matrix is bitwise symmetric with exactly 1.0f on the diagonal
 *                and values in [0, 1] (min(., 1) against rounding; two identical samples give exactly 1)
 *   support      support(a,i) = number of samples b != a of the set with a center of type t_ai within tolerance (<=) of x_ai
 *   clusters     Taylor-Butina: adj(a,b) = a != b and sim(a,b) >= threshold on the fp32 values as written, count(a) = sum_b adj(a,b);
 *                samples are visited in the order (-count, index); an unassigned sample becomes the centroid of a new cluster (ids
 *                in order of creation) and takes every still unassigned neighbour; counts are not updated as samples leave
 *   consensus    of cluster c with centroid sample m, per center i of m: the members b of c ascending (m included) each give their
 *                nearest center of type t_mi within tolerance of x_mi (ties: the lowest j); cnt_i counts them, the consensus
 *                position is their fp32 sum in that order divided by cnt_i
 * P sets per call.  HOST arrays set_ptr [P+1] (set p owns samples [set_ptr[p], set_ptr[p+1])) and center_ptr [S+1] (sample s owns
 * centers [center_ptr[s], center_ptr[s+1])), copied before the call returns.  DEVICE arrays: dev_x [N,3], dev_type [N] int32 in;
 * out dev_sim [sum S_p^2] (set p's S_p x S_p matrix row-major, the sets one after the other; NULL: kept in the handle's
 * workspace), dev_support [N] int32, dev_label [S] (cluster id within the set), dev_centroid / dev_size [S] (cluster c of set p
 * sits at slot set_ptr[p] + c: the centroid's sample index within the set and the member count; slots beyond n_clusters hold -1),
 * dev_n_clusters [P], dev_cons_x [N,3] and dev_cons_cnt [N] int32 (filled for the centers of centroid samples, zero elsewhere).
 * Validation on the host before anything is launched (csrc/pf_sset.h): pointers start at 0 and do not decrease, 1 <= S_p <= 1024,
 * 1 <= n_a <= 64, sum S_p^2 <= 2^26, finite options in range -- a failure is PF_ERR_ARG with a message.  The types are on the
 * device: the kernel counts those outside [0, pharm_nf), the host reads the count behind the launches (the call waits for the
 * stream) and reports PF_ERR_ARG; the outputs then mean nothing.
 * The call needs no committed weights and no bound batch, owns its workspace (grown on demand, freed by pf_destroy) and touches no
 * run state: between two sampling runs, inside one, or while a batch is bound, it changes nothing those see.  Every output has
 * the same bits on every run, and a set's outputs do not depend on the other sets of the call. */
#define PF_SSET_MAX_SAMPLES 1024
#define PF_SSET_MAX_CENTERS 64
typedef struct pf_sset_opts { float sigma; float tolerance; float threshold; } pf_sset_opts;
int pf_sample_set_analyze(pf_handle* h, int32_t P, const int32_t* host_set_ptr /*[P+1]*/, const int32_t* host_center_ptr /*[S+1]*/,
                          const float* dev_x /*[N,3]*/, const int32_t* dev_type /*[N]*/, const pf_sset_opts* opts,
                          float* dev_sim /*[sum S_p^2] or NULL*/, int32_t* dev_support /*[N]*/, int32_t* dev_label /*[S]*/,
                          int32_t* dev_centroid /*[S]*/, int32_t* dev_size /*[S]*/, int32_t* dev_n_clusters /*[P]*/,
                          float* dev_cons_x /*[N,3]*/, int32_t* dev_cons_cnt /*[N]*/, pf_stream stream);

/* -- pharmacophore alignment: superpose library entries onto queries and rank them (no reference counterpart) --------
 * A query is (x [n_q,3], t [n_q]) with 1 <= n_q <= 16, a library entry (y [n_l,3], u [n_l]) with 1 <= n_l <= 32; types are integers
 * in [0, pharm_nf) and match exactly.  Options: sigma > 0 (Gaussian width, 1.0), tolerance >= 0 (matching distance, 1.5), refine in
 * 0..16 (refinement rounds, 4), min_area > 0 (smallest |cross product| of a triplet, 1.0 A^2).  Per (query, entry) pair:
 *   seeds        in lexicographic order of (i, j, k, a, b, c): every query triplet i < j < k and ordered triple of distinct entry
 *                centers (a, b, c) with u_a = t_i, u_b = t_j, u_c = t_k; | d(x_i,x_j) - d(y_a,y_b) | <= 2 tolerance and likewise for
 *                (i,k)/(a,c) and (j,k)/(b,c); |(x_j - x_i) x (x_k - x_i)| >= min_area and |(y_b - y_a) x (y_c - y_a)| >= min_area
 *                (collinear triplets fix no rotation).  A seed's transform (R, s) is the proper rotation (det +1) and translation
 *                that minimise sum |R y + s - x|^2 over its three correspondences
 *   overlap      O = sum_p sum_q [t_p == u_q] exp(-|x_p - (R y_q + s)|^2 / (2 sigma^2)), the typed overlap of the sample sets;
 *                the best seed has the largest O, on a tie the earliest in the enumeration order
 *   refinement   from the best seed up to `refine` rounds: weights w_pq = [t_p == u_q] exp(-|x_p - (R y_q + s)|^2 / (2 sigma^2)) at
 *                the current transform, the weighted least-squares proper rotation and translation over all same-type pairs, the
 *                new overlap O'; accepted when O' >= O, otherwise the refinement stops
 *   outputs      sim = O / (O_qq + O_ll - O), at most 1 (O_qq, O_ll: the self overlaps); n_matched = the number of query centers
 *                with a same-type entry center within tolerance (<=) after the transform; n_seeds; the transform as 12 floats, R
 *                row-major then s, mapping the entry's frame into the query's.  n_seeds = 0 (every pharmacophore of one or two
 *                centers, every entry without three non-collinear type-compatible centers): sim = 0, n_matched = 0, the identity
 * The result is the best of a discrete seed set plus a local refinement, not a global optimum.  Rotations are proper: a mirror
 * image is a different pharmacophore.
 * Q queries against L entries per call, every pair.  HOST arrays q_ptr [Q+1] and l_ptr [L+1] (query k owns the centers
 * [q_ptr[k], q_ptr[k+1]) of dev_qx / dev_qtype, entries likewise), copied before the call returns.  DEVICE arrays: in dev_qx [Nq,3],
 * dev_qtype [Nq] int32, dev_lx [Nl,3], dev_ltype [Nl]; out dev_sim, dev_matched, dev_n_seeds [Q,L] row-major and dev_transform
 * [Q,L,12] (NULL: not written; the other outputs are the same either way).
 * Validation on the host before anything is launched (csrc/pf_align.h): Q, L >= 1, Q * L <= 2^24, pointers start at 0 and do not
 * decrease, center counts within the caps, finite options in range -- a failure is PF_ERR_ARG with a message.  The types are on the
 * device: a kernel counts those outside [0, pharm_nf), the host reads the count behind the launches (the call waits for the
 * stream) and reports PF_ERR_ARG; the outputs then mean nothing.
 * The call needs no committed weights and no bound batch, owns its workspace (grown on demand, freed by pf_destroy) and touches no
 * run state: between two sampling runs, inside one, or while a batch is bound, it changes nothing those see.  fp32 throughout;
 * every output has the same bits on every run, and a pair's outputs do not depend on the other pairs of the call. */
#define PF_ALIGN_MAX_QUERY_CENTERS 16
#define PF_ALIGN_MAX_ENTRY_CENTERS 32
typedef struct pf_align_opts { float sigma; float tolerance; int32_t refine; float min_area; } pf_align_opts;
int pf_pharm_align(pf_handle* h, int32_t Q, const int32_t* host_q_ptr /*[Q+1]*/, int32_t L, const int32_t* host_l_ptr /*[L+1]*/,
                   const float* dev_qx /*[Nq,3]*/, const int32_t* dev_qtype /*[Nq]*/, const float* dev_lx /*[Nl,3]*/,
                   const int32_t* dev_ltype /*[Nl]*/, const pf_align_opts* opts, float* dev_sim /*[Q,L]*/, int32_t* dev_matched /*[Q,L]*/,
                   int32_t* dev_n_seeds /*[Q,L]*/, float* dev_transform /*[Q,L,12] or NULL*/, pf_stream stream);

/* -- seeded sampling: start the reverse process from a given pharmacophore (partial diffusion; no reference counterpart) ----------
 * The given sample is noised forward to an intermediate level a, 1 <= a <= T, and only the reverse steps a-1 .. 0 are run: a small
 * a gives close analogues of the seed, a large a loose ones.
 * Arming.  pf_sample_seed_next is optional and comes after a bind.  It arms the NEXT begin on the handle, of any kind:
 * pf_sample_begin, pf_sample_begin_pinned, pf_sample_begin_guided, or a begin made inside a whole-loop entry.  That begin consumes
 * the seed on entry, whether it then succeeds or is rejected (the rule of pf_set_pocket_groups); a whole-loop entry that rejects its
 * own arguments before it reaches its begin leaves the seed armed.  A bind in between discards the seed, and a second call replaces
 * it.  The two arrays are copied into handle-owned run scratch on `stream` (kept and grown like the pin arrays); the caller may free
 * them once the stream has passed the call.
 * Argument errors.  PF_ERR_ARG for a null argument, for a non-finite coefficient, for alpha_a <= 0, for sigma_a < 0, and for
 * feat_norm_constant <= 0.  In each of these cases the handle and any run in progress are untouched.
 * A seeded begin does what the begin does today: the protein is shifted by init_pharm_com, or by its own mean.  Then, in place of
 * "state := noise0", for every graph g and center f:
 *     D[g]  = c_init[g] - (mean of the graph's current protein rows)          the pinned step's reduction, in its order
 *     x[f]  = alpha_a * (seed_x[f] - D[g])              + sigma_a * noise0_x[f]
 *     h[f]  = alpha_a * (seed_h[f] / feat_norm_constant) + sigma_a * noise0_h[f]
 * One rounding per operation, FP contraction off, as in a pinned step.  Then the COM of all centers of the graph is removed from
 * centers and protein, in the reduction order of pf_denoise_step's update.  One launch (k_step_build<MoveSeed>: the move + the generic
 * edge build; k_step_update<MoveSeed> for the width-generic family and every configuration whose next dynamics call builds its own edges).
 * The rest of the run.  The caller passes n_steps = a and the coefficient entries for s = a-1 .. 0.  Nothing else in the run
 * changes: a seeded plain run takes the default path's steps, merged last launch and center hoist included.  The initial frame of
 * a trajectory is the noised seed.  Pins in a seeded pinned run act from the first step on, as today: the begin does not look at
 * the flags.  At most 64 centers per graph can be bound, so the kernels' path for more than 256 centers of a graph is never taken. */
typedef struct pf_seed_coef { float alpha_a; float sigma_a; } pf_seed_coef;   /* alpha / sigma(gamma(a/T)), fp32, computed by the host */
int pf_sample_seed_next(pf_handle* h, const pf_seed_coef* coef, const float* dev_seed_x /*[Nf,3], caller's frame*/,
                        const float* dev_seed_h /*[Nf,pharm_nf], raw rows*/, float feat_norm_constant, pf_stream stream);

/* -- few-step sampling: strided schedules and a second-order multistep move (no reference counterpart) ---------------------------
 * Strided first-order runs need nothing new here: pf_step_coef is computed by the host for any pair of levels (s, t), s < t, and
 * pf_prepare_timesteps / pf_sample take any list of t, so an ancestral or DDIM run over a subset of the levels is pf_sample (or
 * its pinned, guided and seeded forms) with fewer entries, on the default path's launches.
 * The multistep move.  A second-order multistep solver of the probability-flow ODE (DPM-Solver++ 2M for an endpoint output, its
 * noise-prediction twin for a noise output) is, per block of the state (x: coordinates, h: features),
 *     z_s = (cz * z_t + c0 * o_t) + c1 * o_prev
 * with o_t the network's output for that block AS IT IS (noise, or the clean value under an endpoint parameterisation) and
 * o_prev the output of the step before.  All solver knowledge is in the host's coefficients; the device knows this form only.
 * One rounding per operation, FP contraction off.  No noise is drawn or read.  Then the COM of all centers of the graph is
 * removed from centers and protein, in the reduction order of pf_denoise_step's update.
 * History.  The handle keeps one buffer [Nf, 3 + pharm_nf] with the previous outputs, written by the move itself.  It is valid
 * after a multistep step and invalid after every begin, every bind and every other move.  Where c1 == 0 (both blocks are judged
 * on their own) it is not read and may hold anything.  A step with a non-zero c1 and no valid history fails with PF_ERR_STATE
 * before any launch; the run goes on as if the call had not been made.  A non-finite coefficient is PF_ERR_ARG.
 * pf_denoise_step_ms is legal inside a plain run (after pf_sample_begin, seeded or not), and plain and multistep steps may
 * alternate.  Like a pinned step it runs the separate launches -- one more than the default step -- and ends with one launch
 * of its own (k_step_build<MoveMs>: the move + the generic edge build; k_step_update<MoveMs> for the width-generic family and every
 * configuration whose next dynamics call builds its own edges); nothing is computed ahead across it.
 * pf_sample_ms is the whole run: begin with dev_noise0 [Nf, 3 + pharm_nf] (ONE row: the initial draw), n_steps multistep steps,
 * end.  Trajectories have n_steps + 1 frames.  Pinned and guided runs have no multistep move.
 * Few-step QUALITY is a property of trained weights and is not measured by this project. */
typedef struct pf_ms_coef {
    float t;                    /* l_i / T : the timestep fed to the dynamics */
    float cz_x, c0_x, c1_x;     /* coordinates */
    float cz_h, c0_h, c1_h;     /* features */
} pf_ms_coef;
int pf_denoise_step_ms(pf_handle* h, const pf_ms_coef* coef, pf_stream stream);
int pf_sample_ms(pf_handle* h, int32_t n_steps, const pf_ms_coef* host_coef, const float* dev_noise0 /*[Nf,3+pharm_nf]*/,
                 const float* dev_init_pharm_com /*[B,3] or NULL*/, float feat_norm_constant,
                 float* dev_x0 /*[Nf,3]*/, float* dev_h0 /*[Nf,pharm_nf]*/,
                 float* dev_traj_x /*[n_steps+1,Nf,3] or NULL*/, float* dev_traj_h /*[n_steps+1,Nf,pharm_nf] or NULL*/, pf_stream stream);

/* -- scoring: how plausible are GIVEN pharmacophores for the bound pockets (the per-level terms of PharmacophoreDiff.forward,
 *    pharmacodiff.py:162-243, per graph and at levels the caller chooses; the reference reduces them to batch means) -----------
 * The candidates are the centers of the bound batch: graph g's candidate has pharm_ptr[g+1] - pharm_ptr[g] centers, positions
 * dev_pharm_x0 in the CALLER's frame (the frame of the bound pocket coordinates), rows dev_pharm_h0 the raw type one-hots
 * (divided by feat_norm inside).  For every level l = 0 .. n_levels-1, in order, with t = host_levels[l].t_int (0 <= t <= T):
 *   prepare   per graph the COM of the clean centers is taken off the centers and off the BOUND pocket coordinates (:176-183; never
 *             off what the level before left), z_t = alpha[t] x0 + sigma[t] eps for coordinates and features (:186-197; one rounding
 *             per operation) with eps = row l of dev_noise in the sampler's layout, and the COM of the noised centers is removed
 *             from centers and pocket when remove_com (:199-205)
 *   dynamics  the inference forward at the uniform timestep t / T -- the handle's inference family at every supported width, conv
 *             layer 0's per-timestep tables of all levels made up front (64 timesteps per launch), a pocket-group claim of the
 *             bind honoured (copies of a pocket share conv layer 0's protein->protein messages at each level).  No training
 *             workspace and no pf_train_set_family
 *   evaluate  per graph, summed over its centers f in a fixed order (the same bits on every run), the four forms of
 *             pf_train_loss_forward_ep WITHOUT any weight or division:
 *               pos   sum |eps_x - dyn_x|^2 (:217), or sum |dyn_x + COM2 - x0c|^2 with endpoint_param_coord (:210-215)
 *               feat  sum |eps_h - dyn_h|^2 (:208), or sum cross_entropy(dyn_h, argmax h0) with endpoint_param_feat (:204-206)
 *               err   sum |x0_pred - x0c|^2 (:219, :235), x0c the clean center shifted by the first COM only
 *               hits  centers whose predicted type (first maximum; :209, :237) is the clean type
 *             dev_terms[l][g] = {pos, feat, err, hits} (when given) and
 *             dev_score[g]    = {sum_l w_pos[l] * pos, sum_l w_feat[l] * feat}, added in level order; the first level STORES, so
 *             dev_score need not be initialised.  Nothing is divided by the number of centers: the caller normalises.
 * The whole call is enqueued on `stream` without host synchronisation, like pf_sample; a level costs the forward's launches plus
 * two small ones (k_score_prepare, k_score_eval: one workgroup per graph).  Everything is checked before anything is launched:
 * PF_ERR_ARG for a null argument (dev_terms may be NULL), n_levels < 1, n_timesteps < 1, a t_int outside 0..T, feat_norm <= 0, a
 * batch without centers, pharm_nf > 8, a false pocket-group claim about device rows (its verdict is waited for here, as the first
 * sharing call of the batch would); PF_ERR_STATE without a batch and while a sampling run holds the handle -- from any
 * pf_sample_begin* (or whole-loop entry) until the next bind: the run's state is the handle's state, and the run goes on
 * unharmed after the refusal.
 * What the call leaves: the sampling state machine as it was (no run; a seed armed with pf_sample_seed_next stays armed), and the
 * coordinates held by the handle are the bound ones again, so a sampling run made afterwards gives the bits it gives without the
 * call in front.  A kept pf_train_forward / pf_train_loss_forward does NOT survive (unlike behind pf_dynamics_forward, which
 * leaves the flag alone): the levels overwrite the coordinates and dynamic edges a backward would read, so a backward call
 * afterwards is PF_ERR_STATE.  The score is no likelihood: it has no L_0 term, no prior term and no size prior -- totals compare
 * candidates of one size, across sizes divide by the number of centers. */
typedef struct pf_score_level { int32_t t_int; float w_pos; float w_feat; } pf_score_level;   /* host */
int pf_score(pf_handle* h, const float* dev_pharm_x0 /*[Nf,3], caller's frame*/, const float* dev_pharm_h0 /*[Nf,pharm_nf] raw one-hots*/,
             int32_t n_levels, const pf_score_level* host_levels, const float* dev_noise /*[n_levels, Nf, 3+pharm_nf], x columns first*/,
             const float* dev_alpha /*[T+1]*/, const float* dev_sigma /*[T+1]*/, int32_t n_timesteps, float feat_norm, int32_t remove_com,
             int32_t endpoint_param_coord, int32_t endpoint_param_feat,
             float* dev_score /*[B,2]*/, float* dev_terms /*[n_levels,B,4] or NULL*/, pf_stream stream);

/* -- training step: gradients of the dynamics (autograd through PharmRecDynamicsGVP.forward, ------
 *    dynamics_gvp.py:131-185, as used by PharmacophoreDiff.forward / training_step, pharmacodiff.py:162-276)
 * Parameters and gradients are exchanged as ONE flat fp32 vector in the reference's state-dict order
 * (pf_param_layout enumerates name / offset / numel; a tensor's gradient sits at the offset of the tensor).
 * pf_train_forward  = the boundary function in train() mode: same outputs as pf_dynamics_forward plus GVPDropout
 *                     (gvp.py:118-149, rate dropout_p, counter-based masks from `seed`) at the two call sites of every
 *                     conv layer; keeps each layer's input state for the backward pass.
 * pf_train_backward = d(loss)/d(parameters) given d(loss)/d(eps_h), d(loss)/d(eps_x) of that forward.  The loss itself
 *                     (pharmacodiff.py:208-232) is elementwise on eps and is the caller's.
 * The optimiser is the caller's too (optim.Adam, pharmacodiff.py:253): after a step, push the new values with
 * pf_set_weight + pf_commit_weights. */
int pf_param_count(pf_handle* h, int64_t* n_params, int32_t* n_tensors);
int pf_param_layout(pf_handle* h, int32_t index, const char** name, int64_t* offset, int64_t* numel);
int pf_train_forward(pf_handle* h, const float* dev_prot_x /*[Np,3] or NULL*/, const float* dev_pharm_x /*[Nf,3]*/,
                     const float* dev_pharm_h /*[Nf,pharm_nf]*/, const float* dev_t /*[B]*/, float dropout_p, uint32_t seed,
                     float* dev_eps_h, float* dev_eps_x, pf_stream stream);
int pf_train_backward(pf_handle* h, const float* dev_g_eps_h /*[Nf,pharm_nf]*/, const float* dev_g_eps_x /*[Nf,3]*/,
                      float* dev_grad /*[n_params]*/, pf_stream stream);
/* pf_train_backward + the gradient of the same scalar w.r.t. the inputs of that forward: the center coordinates and the center
 * feature rows as passed to pf_train_forward.  Either output pointer may be NULL; with both NULL the call IS pf_train_backward.
 * Every element of a requested output is stored (nothing is accumulated), on the caller's stream, the same bits on every run.
 * The edge sets are piecewise constant in the coordinates and carry no gradient (as torch on the reference); t and the protein
 * coordinates get none.  On the width-generic training leg (pf_train_set_family(h, PF_TRAIN_FAMILY_WIDE): fp32, every supported
 * width, a 128 / 16 handle included), and on the tuned family once pf_train_set_input_grads(h, 1) is set (fp32): without that
 * switch a non-NULL output pointer on the tuned family is PF_ERR_ARG, nothing is launched and the kept forward stays good for
 * pf_train_backward.  The forward keeps its own copy of the coordinates: the caller's buffers need not outlive pf_train_forward.
 * The parameter gradient has the bits pf_train_backward gives, with the switch on or off. */
int pf_train_backward_inputs(pf_handle* h, const float* dev_g_eps_h, const float* dev_g_eps_x, float* dev_grad /*[n_params]*/,
                             float* dev_g_pharm_x /*[Nf,3] or NULL*/, float* dev_g_pharm_h /*[Nf,pharm_nf] or NULL*/, pf_stream stream);
/* The gradients w.r.t. the inputs ALONE: pf_train_backward_inputs without the parameter gradient (what a guided sampling step
 * needs).  Nothing of the weight-gradient work is done -- the workgroups' gradient copies are neither cleared nor summed, and the
 * gradient kernels run in a form without their weight-gradient products.  Same preconditions as pf_train_backward_inputs (wide
 * family, or the tuned one with pf_train_set_input_grads; a kept pf_train_forward; it may be called any number of times on one
 * forward, before or after a full backward); at least one output must be non-NULL (else PF_ERR_ARG).  Every element of a
 * requested output is stored, with the bits pf_train_backward_inputs stores.  On the tuned family the reduces and the encoders'
 * protein tiles are left out, but the gradient kernels run in their full form: their weight-gradient products land in the
 * workgroups' gradient copies, which nobody sums (a later full backward stores every copy it reads anew). */
int pf_dynamics_input_vjp(pf_handle* h, const float* dev_g_eps_h /*[Nf,pharm_nf]*/, const float* dev_g_eps_x /*[Nf,3]*/,
                          float* dev_g_pharm_x /*[Nf,3] or NULL*/, float* dev_g_pharm_h /*[Nf,pharm_nf] or NULL*/, pf_stream stream);
/* The loss around the dynamics, fused (PharmacophoreDiff.forward, pharmacodiff.py:162-243; pf_train_loss_forward: the noise
 * parameterisation of both outputs, pf_train_loss_forward_ep: every combination of endpoint_param_coord /
 * endpoint_param_feat, see below): per graph the COM of the clean centers is taken
 * off the centers and the bound pocket (:176-183), z_t = alpha_t x0 + sigma_t eps with alpha / sigma read from the caller's
 * tables at t_int (:186-197: dev_alpha[k] = alpha(gamma(k / T)), likewise sigma), the COM of the noised centers is removed
 * when remove_com (:199-205), the dynamics run in train() mode (pf_train_forward), and dev_out receives
 *   [0] pos loss  [1] feat loss  (:208-232, weighted by 1 - t when weighted_loss)
 *   [2] position error  [3] weighted position error  [4] accuracy  [5] weighted accuracy  (:234-241)
 *   [6] total loss = [0] + [1]  [7] total error = [2] + 1 - [4]  [8] weighted total error = [3] + 1 - [5]  (what
 *       training_step / validation_step derive, :274-277, :303-306).
 * dev_pharm_h0 are the raw feature one-hots (divided by feat_norm inside).  The protein coordinates are the bound ones.
 * pf_train_loss_forward_ep takes the two parameterisation flags of the reference's configuration (independent of each
 * other; pf_train_loss_forward is its (0, 0) call and computes the same bits).  With wl = 1 - t when weighted_loss, else 1,
 * per center f of graph g the four forms are
 *   endpoint_param_coord 0  pos loss term |eps_x - dyn_x|^2 (:217); position error |(x_t - sigma_t dyn_x) / alpha_t - x0|^2 (:219)
 *   endpoint_param_coord 1  the dynamics predict the clean center: x_pred = dyn_x + COM taken off the noised centers (added
 *                           only when remove_com), pos loss term |x_pred - x0|^2 (:210-215), which is also the position error
 *   endpoint_param_feat 0   feat loss term |eps_h - dyn_h|^2 (:208); predicted type argmax (h_t - sigma_t dyn_h) / alpha_t (:209)
 *   endpoint_param_feat 1   the dynamics predict the type logits: feat loss term cross_entropy(dyn_h, argmax h0) (:204-206),
 *                           predicted type argmax dyn_h
 * with x0 the COM-removed clean center; the terms times wl are summed and divided by eps.numel() (:226-232: Nf * 3 and
 * Nf * pharm_nf, the cross-entropy's too), the metrics are as above (:234-241).  The backward calls serve every form.
 * pf_train_loss_backward(g_pos, g_feat) = d(g_pos * pos loss + g_feat * feat loss)/d(parameters), the two upstream
 * scalars read from device memory; it consumes the state of the forward (one backward per forward).
 * pf_train_loss_backward_out takes the upstream gradient of all nine outputs instead (what autograd hands the node that
 * produced dev_out): g_pos = g_out[0] + g_out[6], g_feat = g_out[1] + g_out[6]; the metrics' entries are ignored. */
int pf_train_loss_forward(pf_handle* h, const float* dev_pharm_x0 /*[Nf,3]*/, const float* dev_pharm_h0 /*[Nf,pharm_nf]*/,
                          const int32_t* dev_t_int /*[B]*/, const float* dev_eps_x /*[Nf,3]*/, const float* dev_eps_h /*[Nf,pharm_nf]*/,
                          const float* dev_alpha /*[>= max t_int + 1]*/, const float* dev_sigma, int32_t n_timesteps, float feat_norm,
                          int32_t remove_com, int32_t weighted_loss, float dropout_p, uint32_t seed, float* dev_out /*[9]*/,
                          pf_stream stream);
int pf_train_loss_forward_ep(pf_handle* h, const float* dev_pharm_x0 /*[Nf,3]*/, const float* dev_pharm_h0 /*[Nf,pharm_nf]*/,
                             const int32_t* dev_t_int /*[B]*/, const float* dev_eps_x /*[Nf,3]*/, const float* dev_eps_h /*[Nf,pharm_nf]*/,
                             const float* dev_alpha /*[>= max t_int + 1]*/, const float* dev_sigma, int32_t n_timesteps, float feat_norm,
                             int32_t remove_com, int32_t weighted_loss, int32_t endpoint_param_coord, int32_t endpoint_param_feat,
                             float dropout_p, uint32_t seed, float* dev_out /*[9]*/, pf_stream stream);
int pf_train_loss_backward(pf_handle* h, const float* dev_g_pos /*[1]*/, const float* dev_g_feat /*[1]*/,
                           float* dev_grad /*[n_params]*/, pf_stream stream);
int pf_train_loss_backward_out(pf_handle* h, const float* dev_g_out /*[9]*/, float* dev_grad /*[n_params]*/, pf_stream stream);
/* the flat parameter vector on the device: set = copy in + refresh the packed MFMA-fragment weights by a device gather
 * (what an optimiser step calls instead of 245 x pf_set_weight + pf_commit_weights); get = copy out */
int pf_set_flat_params(pf_handle* h, const float* dev_flat /*[n_params]*/, pf_stream stream);
int pf_get_flat_params(pf_handle* h, float* dev_flat /*[n_params]*/, pf_stream stream);
/* one fused Adam step (torch.optim.Adam semantics: L2 weight decay into the gradient, bias correction, no amsgrad;
 * pharmacodiff.py:253) on the caller's flat vectors [n_params], followed by pf_set_flat_params(dev_params).
 * step counts from 1. */
int pf_adam_step(pf_handle* h, float* dev_params, const float* dev_grad, float* dev_exp_avg, float* dev_exp_avg_sq,
                 int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay, pf_stream stream);
/* The guarded optimiser step: pf_adam_step's Adam on gi = grad[i] * grad_scale * coef, behind a norm of the whole gradient
 * that is taken on the device (sum of squares in fp64, fixed reduction order: the same input gives the same bits).
 *   clip_mode PF_CLIP_NONE   coef = 1
 *             PF_CLIP_NORM   coef = min(1, clip / (grad_scale * norm + 1e-6f)), fp32: torch.nn.utils.clip_grad_norm_(max_norm = clip)
 *             PF_CLIP_VALUE  coef = 1, gi clamped to [-clip, clip] behind the scale: torch.nn.utils.clip_grad_value_
 * then the L2 weight decay and Adam as in pf_adam_step.  grad_scale: 1 / N for a gradient summed over N micro-batches.
 * A non-finite norm (some grad[i] is inf or NaN, or the norm exceeds the fp32 range) SKIPS the step: parameters, both moments,
 * the EMA vector and the handle's weights keep their bits, the skipped counter goes up, the applied counter does not.  The bias
 * corrections use the applied count, which lives in the state block: the host needs no synchronisation to learn of a skip.
 * dev_ema (or NULL): ema[i] += (1 - ema_decay) * (new parameter - ema[i]) in the same pass.
 * dev_state: PF_OPTIM_STATE_BYTES of caller-owned device memory, 8-byte aligned, set up by pf_optim_state_init (applied_steps:
 * 0 for a fresh run, the checkpoint's count on a resume):
 *   byte  0  int64  applied steps            byte  8  int64  skipped steps
 *   byte 16  float  norm of the last call's scaled gradient (grad_scale * norm)
 *   byte 20  float  coef of the last call (0 when it was skipped)
 *   byte 24  int32  1 iff the last call's norm was finite (the step was applied)
 *   byte 28  float  1 - beta1^applied, byte 32  float  sqrt(1 - beta2^applied) of the last applied step; the rest is reserved.
 * Options are checked on the host before anything is enqueued (all finite, 0 <= beta < 1, clip >= 0, 0 <= ema_decay < 1,
 * grad_scale > 0, a known clip_mode): PF_ERR_ARG, nothing touched.  pf_adam_step_guarded then refreshes the handle's weights from
 * dev_params like pf_adam_step.  pf_debug_optim_step runs the same launches on caller vectors of any length n >= 1 and leaves
 * the handle's weights alone; pf_debug_optim_chunk is the number of elements one workgroup reduces (tests reach its edges). */
#define PF_CLIP_NONE 0
#define PF_CLIP_NORM 1
#define PF_CLIP_VALUE 2
#define PF_OPTIM_STATE_BYTES 64
typedef struct pf_optim_opts {
    float lr, beta1, beta2, eps, weight_decay, grad_scale;
    int32_t clip_mode;
    float clip, ema_decay;
} pf_optim_opts;
int pf_optim_state_init(pf_handle* h, void* dev_state, int64_t applied_steps, pf_stream stream);
int pf_adam_step_guarded(pf_handle* h, float* dev_params, const float* dev_grad, float* dev_exp_avg, float* dev_exp_avg_sq,
                         float* dev_ema, void* dev_state, const pf_optim_opts* opts, pf_stream stream);
int pf_debug_optim_step(pf_handle* h, int64_t n, float* dev_params, const float* dev_grad, float* dev_exp_avg,
                        float* dev_exp_avg_sq, float* dev_ema, void* dev_state, const pf_optim_opts* opts, pf_stream stream);
int pf_debug_optim_chunk(void);
/* Arithmetic of the training step's dense Linears.  The reference trains in fp32 (pharmacodiff.py:162-263; gvp.py:96,101 force
 * .float()) and PF_TRAIN_F32 -- the default, and the only mode the parity tests against the reference's gradients use -- does
 * the same.  PF_TRAIN_BF16 (BASELINE config 5's "bf16" leg; no reference counterpart) runs to_feats_out and
 * scalar_to_vector_gates of the message chains' forward and the corresponding products of every gradient kernel (input and
 * weight gradients of to_feats_out; in the message chains also of the gates) on bf16 matrix instructions: operands rounded to
 * nearest even, fp32 accumulation.  Master weights, saved activations, LayerNorm, the vector channel, scatter sums, the loss
 * and the optimiser stay fp32.  Contract (tests/test_gpu_train.py): per-tensor gradient cosine >= 0.999 against the fp32
 * path.  Applies to the following pf_train_* calls; a forward of one precision cannot be followed by a backward of the other. */
#define PF_TRAIN_F32 0
#define PF_TRAIN_BF16 1
int pf_train_set_precision(pf_handle* h, int32_t precision);
int pf_train_get_precision(pf_handle* h, int32_t* precision);
/* Kernel family of the training step.  PF_TRAIN_FAMILY_TUNED -- the default -- is the gradient path specialised to
 * n_hidden_scalars 128 / vector_size 16; at other widths every pf_train_* entry is refused.  PF_TRAIN_FAMILY_WIDE runs
 * pf_train_forward / _backward, pf_train_loss_forward / _forward_ep and pf_train_loss_backward / _backward_out on the
 * width-generic kernels (training form of the wide forward, gradient kernels of their own) at every width pair pf_create accepts,
 * fp32 only: together with PF_TRAIN_BF16 it is PF_ERR_ARG, in either order.  A 128 / 16 handle takes it like any other (the A/B
 * against the tuned gradients): its inference stays on the tuned kernels, and the packing the wide forward needs is made from
 * the flat parameter vector on first use and whenever the weights changed.  The leg that is switched away from gives its training
 * workspace back.  The
 * limits of the gradient path hold for both families (at most 4 GVPs per chain, 3 update GVPs, pharm_nf <= 8, rec_nf <= 16,
 * n_convs <= 4).  Under the wide family the dropout multipliers have n_hidden_scalars + vector_size columns per node instead of
 * 144 (pf_debug_set_dropout_masks, pf_debug_dropout_mask).  Switching drops a kept forward: a backward then is PF_ERR_STATE.
 * Inference is untouched by the switch. */
#define PF_TRAIN_FAMILY_TUNED 0
#define PF_TRAIN_FAMILY_WIDE 1
int pf_train_set_family(pf_handle* h, int32_t family);
int pf_train_get_family(pf_handle* h, int32_t* family);
/* Input gradients on the tuned family (off after pf_create).  On, with PF_TRAIN_FAMILY_TUNED and PF_TRAIN_F32 selected,
 * pf_train_backward_inputs fills dev_g_pharm_x / dev_g_pharm_h, pf_dynamics_input_vjp runs the tuned backward without a parameter
 * gradient, and pf_sample_begin_guided / pf_denoise_step_guided / pf_sample_guided accept the handle: a guided step is then the
 * tuned training forward at dropout 0, k_guide_grad, the tuned inputs-only backward and the sampler update.  How: the level-0
 * launch of every conv layer's message chains (k_bwd_edge_level) also leaves dL/d(x_src - x_dst) per edge slot, which one launch
 * sums per center in a fixed order (fp64 lanes, no atomics: the same bits on every run); the encoders' backward stores
 * dL/d(feature rows).  With PF_TRAIN_BF16 selected these entries answer PF_ERR_ARG before anything is launched (call
 * pf_train_set_precision(h, PF_TRAIN_F32)); the kept forward stays usable.  The switch means nothing on the wide family, which
 * always has input gradients, and changes no bit of a parameter gradient.  It owns its buffer ([n_convs][edge slots][3] floats,
 * cleared per pass, grown like a run's scratch), released when switched off (which waits for the device).  A guided run records
 * the family and the switch it began on: a step after either changed is PF_ERR_STATE.  Off, every entry behaves as before the
 * switch existed.  on must be 0 or 1 (else PF_ERR_ARG; PF_ERR_ARG also for a NULL handle). */
int pf_train_set_input_grads(pf_handle* h, int32_t on);
int pf_train_get_input_grads(pf_handle* h, int32_t* on);
/* tests: make the following pf_train_forward / pf_train_backward calls on this batch use the given multipliers
 * [n_convs][2][N][144] -- under PF_TRAIN_FAMILY_WIDE [n_convs][2][N][n_hidden_scalars + vector_size] -- (layout of
 * pf_debug_dropout_mask) instead of the built-in generator; NULL restores it.  The library cannot see the buffer's size.  The
 * buffer must stay alive until the backward call has finished. */
int pf_debug_set_dropout_masks(pf_handle* h, const float* dev_masks);
/* the {0, 1/(1-p)} multipliers pf_train_forward applies in conv layer `layer` (which: 0 message dropout, gvp.py:518;
 * 1 residual dropout, gvp.py:529): dev_out[node][144] = 128 scalar features then 16 vector channels, global node ids
 * (protein atoms first). */
int pf_debug_dropout_mask(pf_handle* h, int32_t layer, int32_t which, float dropout_p, uint32_t seed,
                          float* dev_out /*[N,144]*/, pf_stream stream);

/* -- introspection for tests / profiling ----------------------------------------------------- */
/* edges of the last dynamics call; etype: 0 ff, 1 pf, 2 fp, 3 pp; ids are ntype-local (reference
 * convention).  host_src == NULL returns the count.  Synchronises `stream`. */
int64_t pf_debug_get_edges(pf_handle* h, int32_t etype, int32_t* host_src, int32_t* host_dst, int64_t capacity,
                           pf_stream stream);
/* run one GVPMultiEdgeConv layer (gvp.py:459-538) on caller-provided node features, on the edges
 * built from the given coordinates: tests the conv kernels with non-zero vector inputs. */
int pf_debug_conv_layer(pf_handle* h, int32_t layer, const float* dev_prot_x, const float* dev_pharm_x,
                        const float* dev_h_prot /*[Np,128]*/, const float* dev_v_prot /*[Np,16,3]*/,
                        const float* dev_h_pharm, const float* dev_v_pharm,
                        float* dev_out_h_prot, float* dev_out_v_prot, float* dev_out_h_pharm, float* dev_out_v_pharm,
                        pf_stream stream);
/* per-kernel timing with HIP events recorded on the caller's stream around every launch of the
 * selected kernel classes (bit k of kernel_mask): 0 encode, 1 build_edges (0 and 1 share one launch unless
 * either is being timed), 2 edge_msg (one wave per tile), 3 node_update (one wave per tile), 4 noise_head,
 * 5 step_update (in a pf_score call: its two kernels, k_score_prepare and k_score_eval), 6 edge_msg_coop, 7 node_update_coop (four waves per tile: launches with few tiles),
 * 8 edge_msg_coop of the last conv layer (when n_convs > 1).  pf_profile_read synchronises `stream`, returns the summed device
 * time [ms] and launch count per class since the last read, and resets the counters; pf_profile_enable only changes the
 * mask, so a caller can bracket a subset of its calls (a pair of event records costs ~10 us of stream time). */
#define PF_NUM_KERNEL_CLASSES 9
int pf_profile_enable(pf_handle* h, uint32_t kernel_mask);
int pf_profile_read(pf_handle* h, double* total_ms /*[9]*/, int64_t* launches /*[9]*/, pf_stream stream);
/* The same for the gradient kernels of pf_train_backward (mask bits 9..12 of pf_profile_enable): 0 noise-head backward,
 * 1 node-update backward, 2 edge-message backward (one launch per GVP level), 3 reserved. */
int pf_profile_read_train(pf_handle* h, double* total_ms /*[4]*/, int64_t* launches /*[4]*/, pf_stream stream);
/* work of the last dynamics call: `flops` / `bytes` = reference-equivalent (SURVEY.md 8(d) formulas on the actual
 * edge counts n_edges[4] = ff, pf, fp, pp, every layer dense); `executed_flops` / `executed_edges[n_convs]` = what the
 * kernels compute after dead-work elimination (last layer: pharm side only; layer before it: active atoms only). */
int pf_debug_work(pf_handle* h, double* flops, double* bytes, int64_t* n_edges /*[4]*/, double* executed_flops,
                  int64_t* executed_edges /*[n_convs]*/, pf_stream stream);
/* row / edge counts of the last dynamics call (or of the edges the last pf_denoise_step built): out[8] = ff, pf, fp, static pp edges,
 * "pa" edges (pp edges into active atoms: what the pruned conv layer computes of the pp etype), active atoms, centers, atoms --
 * what a per-launch FLOP count needs (bench.py: roofline.launches) */
int pf_debug_counts(pf_handle* h, int64_t* out /*[8]*/, pf_stream stream);
/* kernel family of the edge-message launch of conv layer `layer` in the last dynamics call (the launch policy depends
 * on the batch: pf_host.cpp LaunchPolicy): *rows_per_wave = 4 or 8 (row-group kernels, pf_rg.hip: k_rg_edge), 16 (16-row
 * items on the four waves of a workgroup, pf_n16.hip: k_n16_edge; 17 = the fused launch k_n16_fused, whose items also
 * compute conv layer 0's node update of their source rows), 32 (one wave per 32-row tile: k_edge_msg) or 128 (four waves per
 * 32-row tile: k_edge_msg_coop / coop2).  layer == n_convs asks about the launch behind the last conv layer's edge messages:
 * when the last call was the dynamics call of a pf_denoise_step whose node update + noise head + sampler update + edge build
 * ran as ONE tail launch (one workgroup per graph): 4 (pf_rg.hip: k_rg_tail, two two-wave items of four centers) or 16
 * (pf_n16.hip: k_n16_tail, PFDYN_TAIL_FORM=n16); 2 when the node + head items and the per-graph sampler update + edge build ran as
 * different workgroups of one launch (pf_rg.hip: k_rg_node_hs_build, the default for small batches; PFDYN_HS_BUILD=0 switches it
 * off); else 0 */
int pf_debug_kernel_family(pf_handle* h, int32_t layer, int32_t* rows_per_wave);
/* Work a denoising step's merged last launch did AHEAD for the next dynamics call (after a pf_denoise_step whose timestep plan was
 * announced; zeros otherwise).  out[0] = "pa" edges (pp edges into the active atoms) of conv layer 0 whose messages the next call will
 * NOT compute -- they were computed ahead and the update + build found their graphs' regions unchanged; out[1] = "pa" edges computed
 * ahead; out[2] = 1 if the centers' encoder outputs and h_src products were left in tables (center hoist), out[3] = centers covered.
 * Also: pf_debug_kernel_family(layer = n_convs + 1) = 1 when the LAST call's ff / fp items started from those tables, (n_convs + 2) = 1
 * when it skipped regions computed ahead, (n_convs + 3) = the item maps of the LAST call's n16 launches: bit 0 conv layer 0 mapped its
 * ff / pf / fp items by arithmetic (k_n16_edge_u), bit 1 the fused launch did (k_n16_fused_u), bit 2 its items started from edge records.
 * Synchronises the stream. */
int pf_debug_ahead(pf_handle* h, int64_t* out /*[4]*/, pf_stream stream);
/* the check of the rows computed ahead (PFDYN_PA_CHECK=1 at pf_create; zeros otherwise), cumulative since the handle's first batch:
 * violations[0] = kept "pa" groups (those a conv-layer-0 launch skipped: j < min(pa_same[g], groups of g)) that the speculative
 * items of the previous step did NOT compute; [1] = kept groups checked; [2] = kept groups of a graph in front of which the group
 * count of the B regions changed between the two calls (where a map over the live counts goes wrong).  Synchronises the stream. */
int pf_debug_pa_check(pf_handle* h, int64_t* violations /*[3]*/, pf_stream stream);
/* the exchange time-outs of k_rg_node_hs_build counted on this handle since it was created (cumulative; pf_sample_status is the
 * product-path check and reports new ones per run).  Synchronises the device. */
int pf_debug_xchg_timeouts(pf_handle* h, int32_t* n);
/* what this process holds through the library's handles right now: live allocations and their bytes, device and pinned memory
 * together (every handle; no handle needed).  Unlike hipMemGetInfo it counts nothing of other processes on the device, so a caller
 * can check that pf_destroy gave everything back: both numbers return to what they were before pf_create. */
int pf_debug_live_memory(int64_t* n_allocations, int64_t* n_bytes);
/* diagnostic: drop_word != 0 makes the producers of the merged launch skip one exchange word (word 0 of center 0), so that its
 * consumer times out; poll_max > 0 shortens the poll bound (default 65,536 rounds) so that a forced time-out costs microseconds.
 * (0, 0) restores the product behaviour.  tests/test_gpu_n16.py: the time-out must surface on the same run. */
int pf_debug_xchg_fault(pf_handle* h, int32_t drop_word, int32_t poll_max);
/* the noise prediction of the last dynamics call of a pf_denoise_step (what its sampler update consumed) */
int pf_debug_last_eps(pf_handle* h, float* dev_eps_h /*[Nf,pharm_nf] or NULL*/, float* dev_eps_x /*[Nf,3] or NULL*/, pf_stream stream);
/* static hoist of conv layer 0's protein-protein messages in the last dynamics call: *rows_per_wave = 0 (not used: training,
 * tile kernels, protein features that are not element one-hots, PFDYN_NO_L0_HOIST=1), 4 / 8 rows per hoisted wave (row-group
 * kernels: pp edges start at their second message GVP) or 16 (n16 kernels: pp AND pf edges start from a type-table row) */
int pf_debug_l0_hoist(pf_handle* h, int32_t* rows_per_wave);
/* One chain of the row-group kernels (pf_rg.hip: rg_gvp / rg_flush / rg_layernorm, 4 rows per wave) on caller-supplied rows,
 * with the committed weights -- the unit-level checker against the reference's own module outputs (gvp.py:89-116, 152-166;
 * dynamics_gvp.py:10-42).  All pointers are device memory; no batch needs to be bound.
 *   kind 0  message chain of conv `layer`, edge type `sub` (0 ff, 1 pf, 2 fp, 3 pp; gvp.py:545-549):
 *           s_in [n][144] = [h_src, rbf], v_in [n][17][3] = [x_hat, v_src]  ->  s_out [n][128], v_out [n][16][3]
 *   kind 1  update chain of conv `layer`, node type `sub` (0 prot, 1 pharm): [n][128], [n][16][3] -> same shapes
 *   kind 2  GVPLayerNorm of conv `layer`: sub = 2 * node type + (0 message_layer_norms, 1 update_layer_norms)
 *   kind 3  NoisePredictionBlock: s_in [n][128], v_in [n][16][3]  ->  s_out [n][pharm_nf] (eps_h), v_out [n][3] (eps_x)
 *   kind 16 / 17  the message / update chain (kinds 0 / 1, same rows) on the n16 kernels' chain code (pf_n16.hip: n16_block,
 *           16 rows per workgroup of four waves); needs n_message_gvps >= 2 */
int pf_debug_chain(pf_handle* h, int32_t kind, int32_t layer, int32_t sub, int32_t n_rows, const float* dev_s_in,
                   const float* dev_v_in, float* dev_s_out, float* dev_v_out, pf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* PFDYN_H */
