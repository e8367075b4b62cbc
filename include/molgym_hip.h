/* molgym_hip.h -- C ABI of the MI355X (gfx950) PPO policy/value hot path.
 *
 * Boundary replaced (reference = gncs/molgym, all paths under /root/reference):
 *   mg_cov_forward      <- CovariantAC.step(observations, actions) with actions given,
 *                          molgym/agents/covariant/agent.py:209-334 (called from
 *                          molgym/ppo.py:26), after parse_observations (:165-197) has
 *                          been done on the host into the padded arrays taken here.
 *   mg_cov_backward     <- autograd of loss.backward(), molgym/ppo.py:131, through the
 *                          same step(); gradients ACCUMULATE into grad_theta exactly as
 *                          .grad does over mini-batches (ppo.py:122-131).
 *   mg_ppo_loss         <- compute_loss arithmetic, molgym/ppo.py:28-52 (float64 seam).
 *   mg_gae              <- DynamicPPOBuffer.finish_path, molgym/buffer.py:74-82 +
 *                          util.discount_cumsum, molgym/tools/util.py:72-87.
 *   mg_adv_normalize    <- DynamicPPOBuffer.get_data, molgym/buffer.py:104-110.
 *   mg_grad_norm_clip   <- util.compute_gradient_norm (util.py:61-69) +
 *                          torch.nn.utils.clip_grad_norm_ (ppo.py:144).
 *
 * All pointers are DEVICE pointers unless a name ends in _host.  No ownership is taken.
 * Every entry point returns 0 on success, a negative MG_E* code otherwise, and never
 * throws; mg_last_error() gives the text.  Launches go to `stream` (a hipStream_t passed
 * as void*), nothing synchronises the device.
 */
#ifndef MOLGYM_HIP_H
#define MOLGYM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_OK 0
#define MG_EINVAL (-1)   /* unsupported / inconsistent configuration */
#define MG_EHIP (-2)     /* HIP runtime error */
#define MG_ENOMEM (-3)   /* workspace too small */

/* len(zs) limit of both agents.  CovariantAC additionally needs len(zs) * num_channels_per_element <= MG_MAX_ZCE: the last atom
 * level's complex mix is a real GEMM of 2 * Z * CE columns and the row / concatenated weight-gradient forms stop at 128. */
#define MG_MAX_Z 16
#define MG_MAX_ZCE 64
/* canvas_size limit of both agents (SchNetAC: molecules of canvas_size + 1 <= 256 atoms).  The CG kernels keep a molecule's
 * atom count in 8 bits of their atom descriptors. */
#define MG_MAX_CANVAS 255

/* Fixed by the build (reference defaults, molgym/tools/arg_parser.py:55-60):
 * maxl = 4, num_cg_levels = 3, num_channels_hidden = 10, num_channels_per_element = 4; the last three are -D parameters
 * of other builds of the same sources (mg_cov_build_params). */
typedef struct mg_cov_cfg {
  int32_t B;            /* samples in the mini-batch                                   */
  int32_t N;            /* canvas_size                                                 */
  int32_t Z;            /* len(zs), zs[0] == 0 is the null symbol                      */
  int32_t zs[MG_MAX_Z]; /* atomic numbers                                              */
  int32_t W;            /* network_width (multiple of 4)                               */
  int32_t G;            /* num_gaussians                                               */
  int32_t TA;           /* total real atoms in the batch  = sum_b n_b                  */
  int32_t TE;           /* total real edges in the batch  = sum_b n_b^2                */
  int32_t has_beta;     /* 1: ExpSO3Distribution(beta); 0: SO3Distribution             */
  float beta;
  float bag_scale;
  float min_distance, max_distance;
} mg_cov_cfg;

const char* mg_last_error(void);
/* MG_ABI_VERSION is bumped whenever an entry point is added / changed or the workspace layout changes; the binding
 * (molgym_amd/_lib.py::_bind) refuses a library whose mg_abi_version() differs, so a stale prebuilt .so is caught by the
 * version and not by a missing symbol.  1: rounds 1-2; 2: mg_cov_channels, mg_cov_sample_ids, channel-major workspace; 3: mg_cov_ppo_step; 4: mg_ppo_epoch_end, mg_adam_step_gated; 5: mg_cov_step_launches; 6: mg_int_ppo_step; 7: mg_cov_build_params (num_cg_levels a build parameter); 8: mg_cov_ppo_step takes `flags`, mg_cov_fold_grads, derived weights first in the workspace; 9: mg_int_ppo_step takes `flags` (MG_STEP_WEIGHTS_CURRENT), derived weights first in the SchNetAC workspace too; 10: mg_int_sample_workspace_bytes, mg_int_sample_ids, mg_int_place, mg_canvas_place; 11: mg_test_gemm, mg_test_gemm_dw; 12: MG_MAX_Z 8 -> 16 (mg_cov_cfg.zs / mg_int_cfg.zs hold 16 entries); 13: mg_set_deterministic, mg_get_deterministic, mg_gemm_dw_ordered_scratch_bytes, mg_test_gemm_dw_ordered; 14: mg_cov_set_ordered, mg_cov_get_ordered (ordered scratch behind the CovariantAC workspace while on); 16: mg_fold_rows; 17: mg_test_gemm_mt; 18: MG_FORM_* bits 3, 4, 7, 11, 17 retired; 19: mg_episode_step; 20: mg_test_gemm_dw_flush, mg_test_gemm_dw_flush_plan; 21: mg_test_catrow_map, the atom cat-mix rows of the levels >= 1 hold the stored columns only (workspace layout); 22: mg_episode_step_rules, mg_episode_draw_formulas, mg_episode_rules; 23: mg_traj_record, mg_traj_status, mg_episode_cut, mg_traj_gae, MG_EP_LOW_REWARD; 24: mg_launch_log_enable, mg_launch_log_report; 25: mg_int_gather_batch; 26: mg_traj_pack, mg_traj_unpack; 27: mg_traj_pair_reward; 28: mg_pair_energy_forces, mg_pair_relax, mg_pair_relax_scratch_bytes; 29: mg_superpose.  */
#define MG_ABI_VERSION 29
int mg_abi_version(void);
/* num_channels_hidden / num_channels_per_element THIS build of the library was compiled for (tools/arg_parser.py:55-60;
 * covariant/agent.py:64,82-83 derive every SO3Tau from them): compile-time constants of the kernels, 10 / 4 by default.
 * Other values are other builds of the same sources (hipcc -DCH=.. -DCE=..); molgym_amd/_lib.py builds / loads them.   */
int mg_cov_channels(int32_t* hidden, int32_t* per_element);
/* the same, with maxl and num_cg_levels (arg_parser.py:55-56).  num_cg_levels is a build parameter too (hipcc -DNLEV=2..4:
 * the level loops, arena and parameter layout follow it; the one-launch-per-level kernels of the small mini-batches are
 * written for 3 and fall back to the general launches otherwise); maxl = 4 is fixed (tables, thread maps, LDS layouts).   */
int mg_cov_build_params(int32_t* hidden, int32_t* per_element, int32_t* maxl, int32_t* num_cg_levels);
/* Tests only: the map between the LOGICAL row [ag: nblk_l | in: 1 | sq: nblk_l] of the atom cat-mix input of the levels >= 1 and
 * the STORED row (ag, in, then the kept sq blocks), per degree l < 5, as the kernels evaluate it.  widths[5]: stored widths;
 * logical_of[l * 32 + cs]: logical column of stored column cs (-1 past the width); stored_of[l * 64 + col] / sign_of[l * 64 + col]:
 * the stored column that serves logical column col and its sign (+1 stored itself, +-1 mirrored onto its partner; -1 / 0: dropped,
 * the block is identically zero).  All host arrays: 5, 160, 320, 320 entries.                                              */
int mg_test_catrow_map(int32_t* widths, int32_t* logical_of, int32_t* stored_of, int32_t* sign_of);

/* ---- deterministic mode (opt-in, off by default) ------------------------------------------------------------------
 * Process-wide switch, read at call time; its initial value is MG_DETERMINISTIC=1 in the environment.  mg_set_deterministic
 * returns the previous value.  Off: nothing changes.  On: mg_int_backward, mg_int_ppo_step, mg_grad_norm_clip and
 * mg_ppo_epoch_end use no float atomics and no side stream -- the same inputs give the same bits on every run and however the
 * step is issued.  Weight gradients take the ordered two-pass GEMM form (partial tiles per fixed row chunk, folded in index
 * order), whose scratch sits behind the SchNetAC workspace: mg_int_workspace_bytes reports the larger size while the switch is
 * on (the offsets of everything else are unchanged) and mg_int_backward / mg_int_ppo_step return MG_ENOMEM for a workspace
 * sized with it off.  mg_int_ppo_step then issues plain stream launches whatever graph_slot says (*used_graph_host = 0).
 * By itself the mode covers SchNetAC only: mg_cov_backward and mg_cov_ppo_step return MG_EINVAL while it is on and
 * mg_cov_set_ordered (below) is off, and so does mg_test_gemm_dw (the ordered form has its own entry point below).       */
int mg_set_deterministic(int on);
int mg_get_deterministic(void);
/* CovariantAC's ordered mode: a SECOND process-wide switch, read at call time, normalised to 0 / 1; its initial value is
 * MG_COV_ORDERED=1 in the environment.  mg_cov_set_ordered returns the previous value.  Off: nothing changes.  On:
 * mg_cov_forward, mg_cov_backward and mg_cov_ppo_step run whatever mg_set_deterministic says, use no float atomic with more
 * than one contributor and no side stream: the general launch path (staged heads, one kernel per encoder stage, the plain
 * DotMatrix layout at every size) with ordered forms of its seven accumulating kernels and the ordered weight-gradient GEMM.
 * Their scratch sits behind the workspace -- 200 CH (TA + TE) bytes for the CG adjoint, plus the largest weight-gradient
 * group -- so mg_cov_workspace_bytes reports the larger size while the switch is on (the offsets of everything else are
 * unchanged) and a workspace sized with it off is MG_ENOMEM.  mg_cov_ppo_step then issues plain stream launches whatever
 * graph_slot says (*used_graph = 0), folds the expanded weight gradients in the step whatever MG_STEP_DEFER_FOLD says (a later
 * mg_cov_fold_grads adds zeros), and MG_CGB_MOL, MG_DW_RIDERS, MG_CB0T are ignored.  A backward on a workspace
 * whose forward ran with the other value of the switch is MG_EINVAL.  The rollout (mg_cov_sample, mg_cov_sample_ids) does
 * not consult the switch: a seed draws what it drew.  mg_grad_norm_clip and mg_ppo_epoch_end follow mg_set_deterministic
 * alone.                                                                                                                */
int mg_cov_set_ordered(int on);
int mg_cov_get_ordered(void);

/* ---- optional kernel-span timing (measurement only) ------------------------------ */
/* on != 0: forward/backward bracket their dominant kernels with HIP events recorded on
 * the launch stream; mg_profile_report writes "name total_ms count" lines (host buffer). */
int mg_profile_enable(int on);
int mg_profile_report(char* buf_host, size_t cap);

/* ---- launch log (tests only) ---------------------------------------------------------- */
/* A log of the kernel launches of the CALLING host thread, off by default.  While it is on, every launch the library
 * issues from that thread -- to the stream, or recorded into the graph of mg_cov_ppo_step / mg_int_ppo_step -- appends one
 * line: the kernel as its call site spells it, template arguments included ("(k_level0_fwd<true, 8>)",
 * "k_catbuild_mfma<false>").  mg_launch_log_enable empties the log and switches it on (on != 0) or off;
 * mg_launch_log_report copies the lines collected since then into a host buffer (MG_ENOMEM if cap is too small).  The
 * log changes nothing about what is launched or how.  Launches made from another thread (autograd runs a backward on
 * its own) are not in the caller's log.                                                                            */
int mg_launch_log_enable(int on);
int mg_launch_log_report(char* buf_host, size_t cap);

/* ---- parameter vector ------------------------------------------------------------- */
/* theta is ONE flat float32 vector.  Slot order and shapes: molgym_amd/layout.py.       */
int mg_cov_num_params(const mg_cov_cfg* cfg, int64_t* num_params);
/* offsets_out[i] = float offset of slot i (n_slots entries, plus the total at the end). */
int mg_cov_param_offsets(const mg_cov_cfg* cfg, int64_t* offsets_out_host, int32_t* n_slots_host);

/* ---- workspace -------------------------------------------------------------------- */
int mg_cov_workspace_bytes(const mg_cov_cfg* cfg, size_t* bytes_host);
/* Look up a named intermediate inside the workspace (tests only): float offset + count.  While mg_cov_set_ordered is on,
   "ord_cg", "ord_phi" and "ord_dw" name the three scratch regions of the ordered mode behind the workspace (each up to the
   start of the next one); with it off they are unknown names like any other. */
int mg_cov_workspace_lookup(const mg_cov_cfg* cfg, const char* name, int64_t* offset_floats_host,
                            int64_t* count_floats_host);

/* ---- forward / backward of CovariantAC.step(obs, actions) ------------------------- */
/* pos      [B][N][3] f32, real atoms first, zero padded (covariant/tools.py:18-31)
 * charges  [B][N] i32 atomic numbers, 0 = padding
 * bags     [B][Z] f32
 * actions  [B][6] f32: focus, element index, distance, ox, oy, oz (agent.py:148-154)
 * leb      [51][1730] f32, feature-major: rows 2q / 2q+1 = Re / Im of Y_q ('qm', q = l*l+l+m) at the
 *          Lebedev-71 points, row 50 = log weight (weights sum to 1); molgym_amd/lebedev.py
 * out      [3][B] f32: logp, ent, v
 * ws       workspace of mg_cov_workspace_bytes(); keeps what backward needs.          */
int mg_cov_forward(const mg_cov_cfg* cfg, const float* theta, const float* pos, const int32_t* charges,
                   const float* bags, const float* actions, const float* leb, void* ws, size_t ws_bytes,
                   float* out, void* stream);
/* Rollout-side step(obs) (actions = None, agent.py:229-292): the four sub-actions are DRAWN on the device as
 * the heads run -- mode 1 = self.training (Categorical / GMM / rejection samplers), mode 2 = evaluation
 * (argmax variants) -- written to actions_out [B][6], and logp / ent / v of the drawn actions to out [3][B].
 * Counter-based RNG keyed by `seed` (the torch RNG stream itself is not reproducible here).               */
int mg_cov_sample(const mg_cov_cfg* cfg, const float* theta, const float* pos, const int32_t* charges,
                  const float* bags, const float* leb, uint64_t seed, int32_t mode, void* ws, size_t ws_bytes,
                  float* actions_out, float* out, void* stream);
/* The same with the random stream of row b keyed by sample_base + sample_stride * b instead of b: a rollout stepped in
 * GROUPS of environments (molgym_amd/ppo.py::_rollout_pipelined overlaps one group's host-side reward,
 * reward.py:36-55, with the other group's policy evaluation; env_container.py:11-74 step_async / step_wait) then draws for
 * every environment what ONE launch over all of them draws.  mg_cov_sample == base 0, stride 1.          */
int mg_cov_sample_ids(const mg_cov_cfg* cfg, const float* theta, const float* pos, const int32_t* charges,
                      const float* bags, const float* leb, uint64_t seed, int32_t sample_base, int32_t sample_stride,
                      int32_t mode, void* ws, size_t ws_bytes, float* actions_out, float* out, void* stream);
/* gout [3][B] f32: dL/dlogp, dL/dent, dL/dv.  grad_theta += dL/dtheta.                 */
int mg_cov_backward(const mg_cov_cfg* cfg, const float* theta, const float* pos, const int32_t* charges,
                    const float* bags, const float* actions, const float* leb, void* ws, size_t ws_bytes,
                    const float* gout, float* grad_theta, void* stream);

/* ---- persistent device canvases of the rollout (replaces the per-step re-parse of every observation,
 * covariant/agent.py:165-197 + covariant/tools.py:8-49, between two steps of an episode) -----------------------------
 * Appends the atom an action row places (to_action_space, agent.py:147-163) to each canvas IN PLACE:
 *   new position = pos64[focus] + (double)(float)(distance * direction)   (origin on an empty canvas),
 *   pos64 / pos32 / charges slot natoms <- it, bags[element] -= 1, natoms += 1   (skipped for a null element or a full canvas)
 * actions [B][6] f32 (mg_cov_sample's actions_out); pos64 [B][N][3] f64 (the environment's own precision), pos32 its f32
 * mirror (what mg_cov_sample / mg_cov_forward read), charges [B][N] i32, bags [B][Z] f32, natoms [B] i32;
 * newpos [B][3] f64 out: the positions placed (what the host hands to the environments); zs_host: HOST array of Z ints. */
int mg_canvas_append(int32_t B, int32_t N, int32_t Z, const int32_t* zs_host, const float* actions, double* pos64,
                     float* pos32, int32_t* charges, float* bags, int32_t* natoms, double* newpos, void* stream);
/* The same commit for the internal-coordinate agent: the atom of the action rows [B][7] (element in column 2) at the float64
 * position newpos [B][3] (mg_int_sample_ids' newpos_out), under the rules of mg_canvas_append.                              */
int mg_canvas_place(int32_t B, int32_t N, int32_t Z, const int32_t* zs_host, const float* actions, const double* newpos,
                    double* pos64, float* pos32, int32_t* charges, float* bags, int32_t* natoms, void* stream);

/* ---- device-resident episodes (replaces the host environment between two policy steps where no reward is needed: the two
 * distance rules environment.py:85-118, the bag decrement :73, the terminal test :81-83 and the reset of what finished,
 * env_container.py reset_if_terminal / ppo.py:201) ---------------------------------------------------------------------------
 * One drawn action per environment on the canvases of mg_canvas_append's layout, updated IN PLACE; takes the place of
 * mg_canvas_append / mg_canvas_place plus the environment's step.  actions [E][cols] f32: cols = 6 (CovariantAC, element in
 * column 1) or 7 (SchNetAC, element in column 2).  newpos [E][3] f64: with compute_pos != 0 (6-column rows only) OUT, the
 * position mg_canvas_append computes, written for every active row; otherwise IN (mg_int_sample_ids' newpos_out).
 * alive [E] i32, episode_no [E] i32: per-environment state.  start_pos64 [E][N][3] f64, start_charges [E][N] i32,
 * start_natoms [E] i32: the canvas each row returns to on reset (all zero for MolecularEnvironment, environment.py:137-140).
 * formulas [F][Z] f32: the bags of the formula cycle (environment.py:134: episode k of a row uses formulas[k % F]).
 * status [E] i32 out: the FIRST rule that applies, in the reference's order (environment.py:49-79):
 *   alive == 0                                                              -> MG_EP_INACTIVE, row untouched (element <- -1)
 *   element outside [0, Z), bags[element] <= 0 for a non-null element (remove_atom_from_formula raises, tools/util.py:33-40),
 *   or natoms outside [0, N]                                                -> MG_EP_ERROR, canvas untouched, alive <- 0
 *   zs[element] == 0                                                        -> MG_EP_STOP
 *   an atom of the row closer than min_atomic_distance to newpos            -> MG_EP_TOO_CLOSE
 *   new Z in {1, 9, 17, 35}, natoms > 0 and no atom with Z outside that set closer than max_solo_distance -> MG_EP_SOLO
 *   natoms == N (no slot for a legal atom; FULL resets, so stepping never leaves such a row)  -> MG_EP_ERROR, as above
 *   otherwise the atom is placed as mg_canvas_place places it: MG_EP_FULL if natoms == N then, else MG_EP_BAG_EMPTY if the bag
 *   sums to 0, else MG_EP_PLACED.
 * Distances are float64, sqrt((dx*dx + dy*dy) + dz*dz), no fused multiply-add; only the row's natoms atoms are read.
 * Every status but INACTIVE, ERROR and PLACED ends the episode, and the row is reset in the same launch: start canvas -> pos64,
 * pos32, charges, natoms; bags <- formulas[(episode_no + 1) % F]; episode_no += 1.  (The atom of a FULL / BAG_EMPTY step is
 * therefore in the record only.)  element [E] i32 out: the element index of the row.  status, element and newpos are the record
 * of the step.  zs_host: HOST array of Z ints.                                                                                 */
#define MG_EP_INACTIVE 0
#define MG_EP_PLACED 1
#define MG_EP_STOP 2
#define MG_EP_TOO_CLOSE 3
#define MG_EP_SOLO 4
#define MG_EP_FULL 5
#define MG_EP_BAG_EMPTY 6
#define MG_EP_ERROR 7
int mg_episode_step(int32_t E, int32_t N, int32_t Z, int32_t F, int32_t cols, int32_t compute_pos, const int32_t* zs_host,
                    double min_atomic_distance, double max_solo_distance, const float* actions, double* newpos, double* pos64,
                    float* pos32, int32_t* charges, float* bags, int32_t* natoms, int32_t* alive, int32_t* episode_no,
                    const double* start_pos64, const int32_t* start_charges, const int32_t* start_natoms, const float* formulas,
                    int32_t* status, int32_t* element, void* stream);

/* ---- the rules of the reference's other three environment classes, in a second entry point (its kernel and
 * mg_episode_step's are the two instantiations of one device body).  mg_episode_step_rules takes the arrays of mg_episode_step plus
 * `rules`, a HOST struct whose pointers are device addresses.  With num_planes = 0, num_refills = 0 and stochastic = 0 it
 * writes exactly what mg_episode_step writes when formula_no holds what episode_no holds.
 * Hull rule (ConstrainedMolecularEnvironment, environment.py:155-171), active when num_planes > 0: planes [P][4] f64, each an
 *   outward unit normal and an offset of one facet of the FIXED scaffold hull, shared by all rows, P <= 2 * MG_MAX_CANVAS.  The
 *   new atom is inside iff max_k(((nx*qx + ny*qy) + nz*qz) + d) <= hull_tol, float64, no fused multiply-add, in that
 *   association; otherwise MG_EP_OUTSIDE, which ends the episode.  The rule sits between STOP and TOO_CLOSE.
 * Refills (RefillableMolecularEnvironment, environment.py:190-207): refills [E] i32, formula_no [E] i32 per row.  The reference
 *   runs ONE formula cycle through resets and refills alike, so formula_no, not episode_no, indexes `formulas`.  A placement that
 *   empties the bag on a canvas that is not full then: MG_EP_REFILLED if refills[e] < num_refills -- the atom is committed,
 *   bags <- formulas[(formula_no + 1) % F], formula_no += 1, refills += 1, the episode goes on -- else MG_EP_BAG_EMPTY.  A
 *   placement that fills the canvas is MG_EP_FULL and consumes no refill (:191-192).  Every episode end sets refills <- 0,
 *   formula_no += 1, episode_no += 1.
 * Sampled formulas (StochasticEnvironment, environment.py:232-249), stochastic != 0 (excludes refills): at every episode end the
 *   row's bag is drawn on the device instead of taken from `formulas`.  One try draws a size in [size_min, size_max) (size_max
 *   when the two are equal; at most 255) and that many symbols i with probability counts[i] / S, S = sum(counts); it is valid iff
 *   sum(count * bond_count[z]) is even (bond counts 1:1, 5:3, 6:4, 7:3, 8:2, 9:1; every symbol with a count needs one).  At most
 *   max_tries (1..64) tries; a row without a valid try gets MG_EP_ERROR and alive <- 0 with its canvas untouched (the reference
 *   would loop forever).  Integer arithmetic only: r = 24 bits of the keyed generator (seed, stream id stream_base +
 *   stream_stride * e, stream number 4, draw try * 256 + k; k = 0 the size, k = 1..size the symbols);
 *   size = size_min + ((r * (size_max - size_min)) >> 24); the symbol is the first i with (r * S) >> 24 < cumulative_count[i].
 * mg_episode_draw_formulas runs the same draw once for all rows (episode 0): bags [E][Z] f32 written and ok[e] <- 1, or
 *   ok[e] <- 0 and the row untouched.  It reads the stochastic fields, seed and stream ids of `rules` only.                     */
#define MG_EP_REFILLED 8 /* the atom was placed and the bag refilled: the episode goes on */
#define MG_EP_OUTSIDE 9  /* the atom lies outside the scaffold hull: the episode ends     */
typedef struct mg_episode_rules {
  int32_t num_refills;           /* >= 0                                                              */
  int32_t num_planes;            /* 0: no hull rule                                                   */
  const double* planes;          /* device [num_planes][4]                                            */
  double hull_tol;               /* >= 0                                                              */
  int32_t* refills;              /* device [E]                                                        */
  int32_t* formula_no;           /* device [E]                                                        */
  int32_t stochastic;            /* != 0: sampled formulas                                            */
  int32_t size_min, size_max;    /* 1 <= size_min <= size_max <= 255                                  */
  int32_t max_tries;             /* 1..64                                                             */
  uint64_t seed;                 /* of this step's draws                                              */
  int32_t stream_base, stream_stride;
  int32_t counts[MG_MAX_Z];      /* the formula the symbols are drawn from, per zs entry              */
} mg_episode_rules;
int mg_episode_step_rules(int32_t E, int32_t N, int32_t Z, int32_t F, int32_t cols, int32_t compute_pos, const int32_t* zs_host,
                          double min_atomic_distance, double max_solo_distance, const float* actions, double* newpos,
                          double* pos64, float* pos32, int32_t* charges, float* bags, int32_t* natoms, int32_t* alive,
                          int32_t* episode_no, const double* start_pos64, const int32_t* start_charges,
                          const int32_t* start_natoms, const float* formulas, int32_t* status, int32_t* element,
                          const mg_episode_rules* rules, void* stream);
int mg_episode_draw_formulas(int32_t E, int32_t Z, const int32_t* zs_host, const mg_episode_rules* rules, float* bags, int32_t* ok,
                             void* stream);

/* ---- trajectory store of device-resident episodes (molgym_amd/rollout.py; csrc/trajectory.inc) ----------------------------
 * The rollout ppo.train reads, recorded where it is sampled.  Environment e's step t of a T-step collect is sample
 * slot = e * T + t -- the order PPOBufferContainer.merge() produces -- in the arrays
 *   s_pos [S][N][3] f32, s_pos64 [S][N][3] f64, s_charges [S][N] i32, s_bags [S][Z] f32, s_actions [S][cols] f32,
 *   s_logp / s_val / s_rew [S] f64, s_status [S] i32                                   (S = E * T; E * T * N * 3 < 2^31).
 * mg_traj_record, between the sampling launch and the episode step: the canvas row (slots beyond natoms as the canvas holds
 *   them), the bag, the action row and logp = out[e], v = out[2 E + e] of the sampling launch's [3][E] block, widened to f64,
 *   go to the row's slot.  A row with alive == 0 writes nothing.
 * mg_traj_status, behind the episode step: s_status[slot] <- status[e] and the rule reward (environment.py:49-64)
 *   s_rew[slot] <- min_reward for TOO_CLOSE / SOLO / OUTSIDE, 0 otherwise (STOP pays 0; an atom-placing status pays the
 *   caller's reward, which the caller writes over the 0).  MG_EP_INACTIVE rows write nothing.
 * mg_episode_cut: for every row with flags[e] != 0 (and alive), s_rew[slot] <- min_reward; where s_status[slot] is PLACED or
 *   REFILLED the open episode ends as in the terminal branch of the step kernels (canvas back to the start structure, bags <-
 *   the next formula of the cycle, natoms, episode_no + 1; with refills / formula_no non-null -- the arrays of
 *   mg_episode_step_rules -- formula_no + 1 and refills <- 0) and s_status[slot] <- MG_EP_LOW_REWARD.  A row whose status was
 *   terminal already only has its reward replaced.  Sampled formulas (mg_episode_rules.stochastic) are not covered.
 * mg_traj_gae: per environment, its T slots backwards; a slot whose status ends an episode starts a new path with bootstrap
 *   0, the tail of a row still open bootstraps with last_val[e]; the recursion and its bits are mg_gae's over the same paths.
 *   num_done[e] <- episodes that ended, len_sum / len_sq[e] <- sum and sum of squares of their lengths; ret at a path's first
 *   slot is its return. */
#define MG_EP_LOW_REWARD 10 /* the caller's reward fell below min_reward: the episode was cut (mg_episode_cut) */
int mg_traj_record(int32_t E, int32_t T, int32_t t, int32_t N, int32_t Z, int32_t cols, const float* pos32, const double* pos64,
                   const int32_t* charges, const float* bags, const float* actions, const float* out, const int32_t* alive,
                   float* s_pos, double* s_pos64, int32_t* s_charges, float* s_bags, float* s_actions, double* s_logp, double* s_val,
                   void* stream);
int mg_traj_status(int32_t E, int32_t T, int32_t t, const int32_t* status, double min_reward, int32_t* s_status, double* s_rew,
                   void* stream);
int mg_episode_cut(int32_t E, int32_t N, int32_t Z, int32_t F, int32_t T, int32_t t, const int32_t* flags, double min_reward,
                   double* pos64, float* pos32, int32_t* charges, float* bags, int32_t* natoms, const int32_t* alive,
                   int32_t* episode_no, const double* start_pos64, const int32_t* start_charges, const int32_t* start_natoms,
                   const float* formulas, int32_t* refills, int32_t* formula_no, int32_t* s_status, double* s_rew, void* stream);
int mg_traj_gae(int32_t E, int32_t T, const int32_t* status, const double* rew, const double* val, const double* last_val,
                double gamma, double lam, double* adv, double* ret, int32_t* num_done, double* len_sum, double* len_sq,
                void* stream);

/* ---- pair-potential reward of a device rollout (molgym_amd/rewards.py: PairReward; csrc/reward.inc) -------------------------
 * mg_traj_pair_reward, BEHIND mg_traj_status and in front of mg_episode_cut: the 12-6 Lennard-Jones interaction of the atom the
 * step placed with the atoms that were there, for every row e whose status[e] is atom-placing (PLACED, FULL, BAG_EMPTY,
 * REFILLED) and whose alive[e] != 0.  The before-canvas is read from the store slot e * T + t that mg_traj_record wrote
 * (s_pos64, s_charges; the live canvas of a FULL / BAG_EMPTY row has been reset by then), the new atom is element[e] (an index
 * into zs, the row of the tables) at newpos[e] of the step record, and natoms_before[e] is the row's atom count BEFORE the step
 * (a device copy of natoms taken in front of the episode step).  four_eps / sigma2: [Z][Z] float64 device tables, 4 eps_ij and
 * sigma_ij^2; a charge is mapped to its column by a search over zs_host (HOST array, passed by value).  In float64, contraction
 * off, exactly this order (the host mirror PairReward.host states the same):
 *   d = q - p_j;  r2 = (dx*dx + dy*dy) + dz*dz;  V_j = 0.0 if r2 > cutoff2 (+inf: no cutoff), else
 *   s = sigma2[a][b_j] / r2;  s3 = (s*s)*s;  V_j = four_eps[a][b_j] * (s3*s3 - s3)
 *   dE = ((V_0 + V_1) + V_2) + ... in canvas slot order, 0.0 for no atoms
 *   reward = -(dE + distance_penalty * sqrt((qx*qx + qy*qy) + qz*qz));  a NaN reward (coincident atoms: inf - inf; a charge
 *   that is not in zs; element / natoms_before out of range) becomes -inf.
 * Such a row gets s_rew[slot] <- reward (the value itself: mg_episode_cut replaces it by min_reward where it cuts),
 * reward_out[e] <- reward and flags[e] <- !(reward >= min_reward), the flag array mg_episode_cut takes.  Every other row gets
 * flags[e] <- 0, reward_out[e] <- 0.0 and nothing of the store is written.  MG_EINVAL: the shape rules of mg_traj_record, a null
 * pointer, NaN min_reward, a negative or non-finite distance_penalty, cutoff2 not > 0. */
int mg_traj_pair_reward(int32_t E, int32_t T, int32_t t, int32_t N, int32_t Z, const int32_t* zs_host, const double* four_eps,
                        const double* sigma2, double distance_penalty, double cutoff2, double min_reward, const int32_t* status,
                        const int32_t* element, const double* newpos, const int32_t* natoms_before, const int32_t* alive,
                        const double* s_pos64, const int32_t* s_charges, double* s_rew, double* reward_out, int32_t* flags,
                        void* stream);

/* ---- energy, gradient and relaxation of whole canvases under the pair potential (molgym_amd/relax.py; csrc/relax.inc) ----------
 * The reference relaxes a sampled structure on the host (minimizer.py: BFGS, gtol 3e-4 on the max-norm of the gradient, 120
 * iterations, optional fixed atoms).  Here E canvases [E][N][3] float64 with charges [E][N] and atom counts natoms [E] are
 * evaluated or relaxed where they lie: one workgroup of 256 threads per canvas, thread i owns atom i.  four_eps / sigma2 / zs_host /
 * cutoff2: as mg_traj_pair_reward.  fixed: [E][N] bytes (non-zero: the atom does not move) or NULL.  Slots >= natoms[e] of the
 * inputs take no part in the arithmetic.  In float64, contraction off, + - * / and comparisons only, exactly this order (the host
 * mirrors PairReward.energy_forces and relax_host state the same):
 *   pair term of atoms i != j, a = index(charges[i]), b = index(charges[j]) (the first position in zs; a charge that is not in zs
 *   gives V = c = NaN):
 *     d = x_i - x_j (per component);  r2 = (dx*dx + dy*dy) + dz*dz
 *     r2 > cutoff2:  V = 0.0, c = 0.0
 *     otherwise      s = sigma2[a][b] / r2;  s3 = (s*s)*s
 *                    V = four_eps[a][b] * (s3*s3 - s3)
 *                    c = (four_eps[a][b] * (6.0*s3 - 12.0*(s3*s3))) / r2
 *   per atom i: E_i is the sequential fold of V over j = 0 .. n-1, j != i, in slot order (the first term starts the fold; no term
 *   gives 0.0); g_i is the same fold of c * d, per component.  A fixed atom's gradient components are set to +0.0 by a select.
 *   reductions over atoms -- E = 0.5 * R(E_i), every dot product R((ax*bx + ay*by) + az*bz), gmax = R_max(larger of the three |g|)
 *   -- use ONE workgroup reduction: 256 slots, slot i holds atom i's value, slots >= n hold +0.0, then v[i] = v[i] + v[i+s] for
 *   s = 128, 64, ..., 1 (R_max: the larger of the two, a NaN wins).
 * mg_pair_energy_forces: energy[e] <- E, grad[e][i][:] <- g_i (slots >= n: +0.0), gmax[e] <- gmax.  A row whose natoms lies outside
 *   0 .. N gets NaN, +0.0 and NaN, and nothing of it is indexed.
 * mg_pair_relax: L-BFGS with m = 8 pairs (s, y), newest first, rho = 1.0 / (s.y), gamma = (s.y) / (y.y) of the newest pair.
 *   before every iteration: gmax <= gtol -> CONVERGED; iterations == max_iter -> MAX_ITER
 *   direction, with a history:  q = g;  newest to oldest: al_t = rho_t * (s_t.q), q = q - al_t * y_t;  r = gamma * q;
 *     oldest to newest: be = rho_t * (y_t.r), r = r + (al_t - be) * s_t;  d = -r;  if g.d < 0 does not hold: drop the history
 *   without a history: d = -g
 *   first trial step a = 1.0 with a history, min(1.0, 0.1 / gmax) without one
 *   trial: x' = x + a * d (a fixed atom keeps x by a select); accept when E(x') <= E + (1e-4 * a) * (g.d); otherwise a = a * 0.5,
 *     at most 30 trials (a NaN energy fails the comparison), then LINE_SEARCH
 *   accepted: s = x' - x, y = g' - g; the pair is stored only when s.y > 1e-12, the oldest pair is dropped first
 *   Energy or gmax not finite at the start: NONFINITE, and the output positions are the input's bytes.  A row whose natoms lies
 *   outside 0 .. N: NONFINITE with NaN energies and gmax, 0 evaluations, the whole row copied, nothing of it indexed.
 *   out_pos64 [E][N][3] <- the relaxed positions (slots >= n: the input's bytes; it may BE pos64), energy0 / energy [E] <- E before
 *   and after, gmax [E], iterations [E], evaluations [E] (energy-and-gradient evaluations, the first one included), status [E].
 *   The history (16 vectors of 3 N doubles) lives in LDS at every canvas size, so mg_pair_relax_scratch_bytes returns 0 and
 *   `scratch` may be NULL; a caller passes what the function reports.
 * MG_EINVAL: E < 1, N outside 1 .. MG_MAX_CANVAS, E * N * 3 >= 2^31, Z outside 2 .. MG_MAX_Z, a null pointer (fixed and scratch
 * excepted), cutoff2 not > 0, max_iter < 0, gtol negative or not finite.  MG_ENOMEM: scratch_bytes below what is reported. */
#define MG_RELAX_CONVERGED 0   /* the only success */
#define MG_RELAX_MAX_ITER 1
#define MG_RELAX_LINE_SEARCH 2 /* 30 trial steps failed */
#define MG_RELAX_NONFINITE 3   /* energy or gradient not finite at the start */
int mg_pair_energy_forces(int32_t E, int32_t N, int32_t Z, const int32_t* zs_host, const double* four_eps, const double* sigma2,
                          double cutoff2, const double* pos64, const int32_t* charges, const int32_t* natoms, const uint8_t* fixed,
                          double* energy, double* grad, double* gmax, void* stream);
size_t mg_pair_relax_scratch_bytes(int32_t E, int32_t N);
int mg_pair_relax(int32_t E, int32_t N, int32_t Z, const int32_t* zs_host, const double* four_eps, const double* sigma2,
                  double cutoff2, const double* pos64, const int32_t* charges, const int32_t* natoms, const uint8_t* fixed,
                  int32_t max_iter, double gtol, double* out_pos64, double* energy0, double* energy, double* gmax,
                  int32_t* iterations, int32_t* evaluations, int32_t* status, void* scratch, size_t scratch_bytes, void* stream);

/* ---- rigid superposition of two sets of canvases (molgym_amd/structure.py; csrc/superpose.inc) -----------------------------------
 * How far a structure moved, for example under mg_pair_relax: B [E][N][3] float64 is laid on A [E][N][3] by the best translation and
 * proper rotation (Horn's quaternion method), over the atoms i < natoms[e] whose select[e][i] != 0 (select NULL: every atom); one
 * workgroup of 256 threads per pair of canvases, one thread per atom, every sum over atoms is the 256-slot reduction of the section
 * above, in which the selected atoms fill the slots 0 .. m-1 in atom order (a selected subset gives the bits of the subset alone).  In float64, contraction off, + - * /, comparisons, selects and sqrt only, in exactly the order that the head of
 * csrc/superpose.inc and the docstring of molgym_amd/structure.py state in the same words (superpose_host is the mirror, the same
 * bits): the selected count m, the centroids, D = R(|a - b|^2), the nine sums M_kl = R(b'_k * a'_l), Horn's symmetric 4 x 4 matrix,
 * exactly 8 cyclic Jacobi sweeps on it, the unit quaternion of the first largest diagonal entry with q0 >= 0, the rotation, and the
 * residuals res = a' - Rot b', from which rmsd and max_deviation are taken (not from the eigenvalue, which cancels for nearly
 * coincident structures).
 *   rmsd [E] <- sqrt(R(res^2) / m), displacement [E] <- sqrt(D / m) (the RMSD without a fit), max_deviation [E] <- the largest |res|,
 *   all three over the selected atoms; rotation [E][9] row-major, centroid_a / centroid_b [E][3]; aligned [E][N][3] or NULL <-
 *   Rot (b - centroid_b) + centroid_a for EVERY atom of the row, selected or not, and the bytes of B in the slots >= natoms[e].  aligned
 *   may BE pos_b (a thread writes only the slot it read); it must not be pos_a.  status [E]:
 *   OK         also a row without a selected atom: the scalars and centroids are 0.0, the rotation is the identity, aligned <- B's bytes
 *   NONFINITE  D, or an entry of the Jacobi working matrix or of its eigenvectors after the last sweep, is not finite (this covers
 *              the centroids and the M_kl), or natoms[e] lies outside 0 .. N (nothing of the row is indexed): NaN in the scalars, the
 *              rotation and the centroids, aligned <- B's bytes for the whole row.
 * MG_EINVAL: E < 1, N outside 1 .. MG_MAX_CANVAS, E * N * 3 >= 2^31, a null pointer (select and aligned excepted), aligned == pos_a. */
#define MG_SUPERPOSE_OK 0
#define MG_SUPERPOSE_NONFINITE 1
int mg_superpose(int32_t E, int32_t N, const double* pos_a, const double* pos_b, const int32_t* natoms,
                 const uint8_t* select /* [E][N] or null: every atom */,
                 double* aligned /* [E][N][3] or null; may be pos_b itself, must not be pos_a */,
                 double* rmsd, double* displacement, double* max_deviation, /* [E] */
                 double* rotation /* [E][9] row-major */, double* centroid_a, double* centroid_b /* [E][3] */,
                 int32_t* status /* [E] */, void* stream);

/* ---- the exchange of the stores under data parallelism (molgym_amd/rollout.py: exchange_layout, pack, unpack_gathered) ------
 * Rank r of `world` records the environments [lo_r, hi_r) = [(r * num_envs) / world, ((r + 1) * num_envs) / world) in a store of
 * its own.  A send block holds MG_TRAJ_SECTIONS = 12 sections: the eleven arrays of the store in the order they lie in it
 * (pos64, logp, val, rew, adv, ret, pos, charges, bags, actions, status), then the int32 atom counts of the samples.  Section s
 * starts at byte sec_off[s] (a multiple of 256; HOST array) and holds sec_words[s] dwords per sample (HOST array); it is sized
 * for the largest share, ceil(num_envs / world) * T samples, so every rank's block has the same `block_bytes` (a multiple of
 * 256) and one all-gather moves the rollout.  `arrays`: HOST array of the 12 device pointers, in section order.
 * mg_traj_pack: the first (hi_rank - lo_rank) * T samples of each of this rank's arrays -> its section of `block`.  The tail
 *   of a section behind a short share and the padding between sections are not written: zero the block once, when it is
 *   allocated.
 * mg_traj_unpack: `gathered` is [world][block_bytes], the blocks in rank order; in ONE launch, rank r's section s goes to
 *   sample offset lo_r * T of arrays[s], (hi_r - lo_r) * T samples -- the arrays of a store of num_envs environments, whose
 *   sample order is g * T + t.  lo_r follows from (num_envs, world) in the kernel.
 * Both are dword copies (a grid stride over rank, section and chunk; no LDS, no atomics): every array is a whole number of
 * dwords and a destination offset is guaranteed no more.  MG_EINVAL: num_envs < world, world < 1, rank outside [0, world),
 * T < 1 or T > capacity, num_envs * capacity * N * 3 >= 2^31 (the gathered store), nsec != 12, a null pointer (an entry of
 * `arrays` included), a section that is not 256-aligned or runs into the next one or past block_bytes. */
#define MG_TRAJ_SECTIONS 12
int mg_traj_pack(int32_t num_envs, int32_t world, int32_t rank, int32_t T, int32_t capacity, int32_t N, int32_t nsec,
                 const int64_t* sec_off, const int32_t* sec_words, const void* const* arrays, void* block, int64_t block_bytes,
                 void* stream);
int mg_traj_unpack(int32_t num_envs, int32_t world, int32_t T, int32_t capacity, int32_t N, int32_t nsec, const int64_t* sec_off,
                   const int32_t* sec_words, const void* gathered, int64_t block_bytes, void* const* arrays, void* stream);

/* ---- mini-batch gather (replaces collect_data_batch, molgym/ppo.py:77-81, on a rollout parked in HBM) ----------------
 * dst[f][b][:] = src[f][idx[b]][:] for nf <= 8 row-major matrices in ONE launch; row_bytes[f] (multiples of 4) are HOST
 * values, src / dst are HOST arrays of device pointers, idx [B] int64 on the device.  ppo.train draws a new permutation
 * every epoch, so every mini-batch is a gather of positions, charges, bags, action rows and the three float64 columns of
 * the loss: seven index_select calls cost more host time than the forward pass's launches.                            */
int mg_gather_rows(int32_t nf, const void* const* src, void* const* dst, const int32_t* row_bytes, const int64_t* idx,
                   int32_t B, void* stream);

/* ---- SchNetAC mini-batch gather (replaces IntRollout.minibatch: SchNetAC._assemble on the host + one upload) -----------
 * The ragged 3B-molecule batch of the rows idx [B] (int64 on the device; NULL: b -> b, then B <= S) of a rollout of S
 * samples parked in HBM: s_pos64 [S][N][3] f64, s_charges [S][N], s_natoms [S], s_bags [S][Z], s_actions [S][7],
 * s_logp / s_adv / s_ret [S] f64.  Written, set-major as mg_int_forward reads them: mol_off [3B+1], edge_off [3B+1]
 * (n (n - 1) ordered pairs per molecule), molZ [MA], molpos [MA][3] f32, bags [B][Z], actions [B][7], logp / adv / ret
 * [B] f64.  Base molecule b holds the n_b = s_natoms[idx[b]] atoms of its canvas at float32(s_pos64); its plus and minus
 * copies hold them and one more atom, element zs_host[round(column 2)] of the action row, at the z-matrix placement of
 * the row (focus = column 1, distance / angle / dihedral = columns 3..5) and at the placement with the dihedral negated:
 * mg_int_place's float64 arithmetic, cast to float32; an empty canvas places at the origin.
 * TA = sum n_b, MA = 3 TA + 2 B, ME = sum (3 n_b^2 + n_b) are HOST values (from the host's mirror of the atom counts);
 * MA != 3 TA + 2 B, a null pointer, B < 1, S < 1, N outside 1..MG_MAX_CANVAS or Z outside 2..MG_MAX_Z return MG_EINVAL and
 * launch nothing.  What only the device can see is ORed into err [1]: 1 = its totals differ from TA / ME, 2 = an atom
 * count outside [0, N] or an index outside [0, S).  A flagged call still writes every output inside its documented size:
 * the MA atoms dealt evenly over the 3B molecules (mol_off[3B] = MA, pair offsets consistent with the sizes and inside
 * ME), zeros for their atoms, the per-sample rows of the clamped indices.  Two launches on `stream`, no synchronisation. */
int mg_int_gather_batch(int32_t B, int32_t N, int32_t Z, int32_t S, int32_t TA, int32_t MA, int32_t ME, const int32_t* zs_host,
                        const int64_t* idx, const double* s_pos64, const int32_t* s_charges, const int32_t* s_natoms,
                        const float* s_bags, const float* s_actions, const double* s_logp, const double* s_adv,
                        const double* s_ret, int32_t* mol_off, int32_t* edge_off, int32_t* molZ, float* molpos, float* bags,
                        float* actions, double* logp, double* adv, double* ret, int32_t* err, void* stream);

/* Input validation of the forward that just ran on `ws`: synchronises `stream`, then MG_EINVAL if the list build found
 * real atoms that are not compacted to the front of their canvas, or cfg.TA / cfg.TE inconsistent with `charges`
 * (the forward itself never synchronises, so it cannot report these).                                              */
int mg_cov_check(const mg_cov_cfg* cfg, const void* ws, size_t ws_bytes, void* stream);

/* ---- head outputs of the forward that just ran (what step()'s `dists` are built from, agent.py:224-286,325-331) ----
 * Packs, sample-major, out of the workspace:  focus logits [B][N] (0 beyond the sample's atoms) | natoms [B] (as f32) |
 * element logits [B][Z] | GMM head [B][2G] (mixture logits, then pre-tanh means) | conditioned orientation
 * coefficients [B][25][CE = 4][2] (q = l*l+l+m) | log Z [B].   out holds B * (N + 1 + Z + 2G + 200 + 1) floats.   */
int mg_cov_head_outputs(const mg_cov_cfg* cfg, const void* ws, size_t ws_bytes, float* out, void* stream);

/* ---- orientation density on caller-supplied points ------------------------------------------------------
 * What dists[-1] of CovariantAC.step()'s return (covariant/agent.py:325-331) evaluates in .log_prob(value) /
 * .prob(value): ExpSO3Distribution (spherical_dists.py:273-286) when has_beta, SO3Distribution (:160-179) otherwise.
 *   coef   [B][25][2] f32 channel-summed coefficients AFTER normalize_alms (so3_tools.py:68-75), q = l*l+l+m
 *   points [S][Bp][3] f32, Bp == B, or 1 to broadcast one grid over the samples; normalised to unit length
 *          inside (cormorant SphericalHarmonics(normalize=True)), a zero vector keeps Y_00 only
 *   logz   [B] f32 (has_beta), empty [B] u8 or NULL (SO3Distribution's uniform density on an empty canvas)
 *   mode   0 = log_prob, 1 = prob, 2 = unnormalised log_prob (has_beta only);  out [S][B] f32               */
int mg_so3_density(int32_t B, int64_t S, int32_t Bp, const float* coef, const float* points, int32_t has_beta,
                   float beta, const float* logz, const uint8_t* empty, int32_t mode, float* out, void* stream);

/* ---- internal-coordinate agent: SchNetAC.step(obs, actions), molgym/agents/internal/agent.py:181-353 ----
 * The schnetpack SchNet embedding is evaluated once over 3B molecules: set 0 = the canvases (n_b atoms), sets 1
 * and 2 = canvas + the new atom placed by zmat.position_atom_helper (internal/zmat.py:96-133, done on the host
 * in float64) at +dihedral / -dihedral.  Molecule m = set * B + b.
 *   mol_off  [3B+1] i32 atom offsets, edge_off [3B+1] i32 ordered-pair offsets (n(n-1) per molecule),
 *   molZ [MA] i32 atomic numbers, molpos [MA][3] f32, bags [B][Z] f32,
 *   actions [B][7] f32: stop, focus, element, distance, angle, dihedral, kappa (agent.py:26,306-308)
 *   out [3][B] f32: logp (masked sum), ent (focus + element), v.                                            */
typedef struct mg_int_cfg {
  int32_t B, N, Z;
  int32_t zs[MG_MAX_Z];
  int32_t W;          /* network_width, multiple of 16                                 */
  int32_t TA;         /* real atoms on the canvases                                    */
  int32_t MA;         /* atoms over all 3B molecules = 3*TA + 2*B                      */
  int32_t ME;         /* ordered pairs over all 3B molecules                           */
  float min_distance, max_distance;
} mg_int_cfg;
int mg_int_num_params(const mg_int_cfg* cfg, int64_t* num_params);
int mg_int_param_offsets(const mg_int_cfg* cfg, int64_t* offsets_out_host, int32_t* n_slots_host);
int mg_int_workspace_bytes(const mg_int_cfg* cfg, size_t* bytes_host);
/* Float offset / count of a named intermediate inside the workspace ("logitF" [TA], "logitE" [B][Z], "cout" [B][3]
 * = phi_continuous output before tanh, "kv" [2][B] kappa logits, ...).  The rollout-side step(obs) of the Python
 * agent reads the distribution parameters of each sub-action through it (internal/agent.py:206-292). */
int mg_int_workspace_lookup(const mg_int_cfg* cfg, const char* name, int64_t* offset_floats_host,
                            int64_t* count_floats_host);
int mg_int_forward(const mg_int_cfg* cfg, const float* theta, const int32_t* mol_off, const int32_t* edge_off,
                   const int32_t* molZ, const float* molpos, const float* bags, const float* actions, void* ws,
                   size_t ws_bytes, float* out, void* stream);
int mg_int_backward(const mg_int_cfg* cfg, const float* theta, const int32_t* mol_off, const int32_t* edge_off,
                    const int32_t* molZ, const float* molpos, const float* bags, const float* actions, void* ws,
                    size_t ws_bytes, const float* gout, float* grad_theta, void* stream);

/* ---- rollout step of the internal-coordinate agent on device-resident canvases (SchNetAC.step_canvas) ----------------------
 * The whole sampling step (agent.py:181-353 with actions = None) on the canvases of mg_canvas_append's layout: the 3B-molecule
 * batch is assembled on the device (a scan over natoms), then forward -> focus draw -> forward -> element draw -> forward ->
 * distance / angle / dihedral draw + float64 z-matrix placement of both dihedral signs -> forward -> kappa draw -> forward, all
 * on `stream`, no host synchronisation, no host-to-device copy.  cfg.TA / MA / ME come from the HOST's mirror of the atom counts;
 * if the device counts disagree, *err_out = 1 (2: a count outside [0, N]) and the step runs on a small placeholder batch instead
 * (the caller raises when it reads the flag).  mode 1 = draw, 2 = evaluation (argmax, means).  Row b reads the random stream
 * (seed, sample_base + sample_stride * b), one stream id per sub-action.  draw_par_host [6] (HOST): half widths and centres
 * of distance / angle / dihedral, the means of the Normals being tanh(out) * half_width + centre.
 * actions_out [B][7] f32 (stop, focus, element, distance, angle, dihedral, kappa), newpos_out [B][3] f64: the position of the
 * atom the row places (dihedral flipped when kappa = 1), out [3][B] f32: logp / ent / v of the drawn rows, err_out [1] i32.
 * ws: mg_int_sample_workspace_bytes; it begins with the forward's workspace (mg_int_workspace_lookup names index it). */
int mg_int_sample_workspace_bytes(const mg_int_cfg* cfg, size_t* bytes_host);
int mg_int_sample_ids(const mg_int_cfg* cfg, const float* theta, const double* pos64, const float* pos32, const int32_t* charges,
                      const float* bags, const int32_t* natoms, uint64_t seed, int32_t sample_base, int32_t sample_stride,
                      int32_t mode, const float* draw_par_host, void* ws, size_t ws_bytes, float* actions_out, double* newpos_out, float* out,
                      int32_t* err_out, void* stream);
/* The z-matrix placement alone (zmat.position_atom_helper, float64, the three nearest atoms in stable order): for the action rows
 * [B][7] on the canvases pos64 [B][N][3] with natoms [B], the new positions with the dihedral kept (plus) and flipped (minus). */
int mg_int_place(int32_t B, int32_t N, const double* pos64, const int32_t* natoms, const float* actions, double* newpos_plus,
                 double* newpos_minus, void* stream);

/* ---- PPO loss, float64 (ppo.py:28-52) --------------------------------------------- */
/* pred [3][B] f32 (logp, ent, v); old_logp, adv, ret [B] f64.
 * stats[6] f64: policy_loss, entropy_loss, vf_loss, total_loss, approx_kl, clip_fraction.
 * gout [3][B] f32 = d total_loss / d pred (may be NULL).                                */
int mg_ppo_loss(int32_t B, const float* pred, const double* old_logp, const double* adv, const double* ret,
                double clip_ratio, double vf_coef, double entropy_coef, double* stats, float* gout,
                void* stream);

/* ---- one PPO mini-batch in one call: step(obs, actions) -> loss -> backward (molgym/ppo.py:124-131) ---------------------
 * What the device-resident update loop of ppo.train does per mini-batch: mg_cov_forward, mg_ppo_loss, mg_cov_backward on the
 * same stream, with
 *   out [3][B], gout [3][B] f32 and stats[6] f64 caller-owned (kept: `out` is what step() returned, gout = d loss / d out);
 *   loss_scale multiplies gout (this rank's share of a data-parallel mini-batch; 1 otherwise);
 *   stats_accum[6] f64 (may be NULL): += loss_scale * stats, atomically -- the epoch's mean of mini-batch means;
 *   gradients ACCUMULATE into grad_theta.
 * graph_slot < 0: ~27 stream launches.  graph_slot in [0, 8): the launches are recorded, the kernel nodes of this host
 * thread's cached graph number graph_slot are updated in place (grids and arguments follow the mini-batch's ragged sizes) and
 * ONE hipGraphLaunch is issued -- ~30 us of host time instead of ~250 (the update loop is host-bound otherwise).  Mini-batches
 * in flight on different streams must use different slots.  Falls back to the stream launches by itself where a graph cannot
 * express the step (side streams of the large configurations); *used_graph_host (may be NULL) reports which form ran.
 * MG_GRAPH=0 in the environment disables the graph form.
 * flags (theta is constant over the mini-batches of a PPO epoch -- the reference steps the optimizer once per epoch,
 * ppo.py:117-146 -- so what depends on theta alone need not be redone per mini-batch):
 *   MG_STEP_WEIGHTS_CURRENT  the derived weight matrices in THIS workspace (they sit first in it, at offsets that do not depend on
 *                            the mini-batch) were written by an earlier call with the same theta: skip their preparation;
 *   MG_STEP_DEFER_FOLD       leave the expanded complex weight gradients accumulating in the workspace instead of folding them
 *                            into grad_theta at the end of the step; the caller folds once per epoch with mg_cov_fold_grads
 *                            (before it reads grad_theta) -- one fold per workspace used.                                      */
#define MG_STEP_WEIGHTS_CURRENT 1
#define MG_STEP_DEFER_FOLD 2
int mg_cov_ppo_step(const mg_cov_cfg* cfg, const float* theta, const float* pos, const int32_t* charges, const float* bags,
                    const float* actions, const float* lebedev, void* workspace, size_t workspace_bytes,
                    const double* old_logp, const double* adv, const double* ret, double clip_ratio, double vf_coef,
                    double entropy_coef, double loss_scale, float* out, float* gout, double* stats, double* stats_accum,
                    float* grad_theta, int32_t graph_slot, int32_t flags, int32_t* used_graph_host, void* stream);
/* grad_theta += the expanded complex weight gradients a workspace accumulated over mg_cov_ppo_step(.., MG_STEP_DEFER_FOLD) calls
 * (and the accumulator is left zero): the per-epoch half of what mg_cov_backward does at the end of every call.             */
int mg_cov_fold_grads(const mg_cov_cfg* cfg, void* workspace, size_t workspace_bytes, float* grad_theta, void* stream);

/* the same for the internal-coordinate agent (mg_int_forward + mg_ppo_loss + mg_int_backward; the loss is evaluated by the last
 * workgroup of the forward's last launch).  flags: MG_STEP_WEIGHTS_CURRENT as above (the derived weight matrices sit first in the
 * workspace, at offsets that do not depend on the batch); this agent has no expanded gradients to fold.                       */
int mg_int_ppo_step(const mg_int_cfg* cfg, const float* theta, const int32_t* mol_off, const int32_t* edge_off,
                    const int32_t* molZ, const float* molpos, const float* bags, const float* actions, void* workspace,
                    size_t workspace_bytes, const double* old_logp, const double* adv, const double* ret, double clip_ratio,
                    double vf_coef, double entropy_coef, double loss_scale, float* out, float* gout, double* stats,
                    double* stats_accum, float* grad_theta, int32_t graph_slot, int32_t flags, int32_t* used_graph_host,
                    void* stream);

/* kernel launches (= graph nodes) of the last mg_cov_ppo_step this host thread issued in graph form; 0 if none (measurement) */
int mg_cov_step_launches(void);

/* ---- GAE-lambda over concatenated trajectories (buffer.py:74-82) ------------------ */
/* path_off [P+1] i32 start offsets; rew, val [T] f64; last_val [P] f64.
 * adv[t] = discount_cumsum(delta, gamma*lam), ret[t] = discount_cumsum(rew ++ last_val, gamma)[:-1] */
int mg_gae(int32_t num_paths, const int32_t* path_off, const double* rew, const double* val,
           const double* last_val, double gamma, double lam, double* adv, double* ret, void* stream);
/* adv <- (adv - mean) / std, population std, no epsilon (buffer.py:104-110).            */
int mg_adv_normalize(int32_t T, double* adv, double* scratch2, void* stream);

/* ---- gradient norm + clip (util.py:61-69, ppo.py:144) ------------------------------ */
/* norm_out[0] = ||g||_2 (f32, device; norm_out must hold 2 floats, [1] is scratch).
 * If max_norm > 0: g *= min(1, max_norm/(norm+1e-6)).                                   */
int mg_grad_norm_clip(int64_t n, float* grad, float max_norm, float* norm_out, void* stream);

/* One Adam update of the flat parameter vector (replaces optimizer.step(), molgym/ppo.py:145, for torch.optim.Adam on the
 * single flat theta): the arithmetic of torch.optim.Adam's foreach implementation in one launch --
 *   grad' = (maximize ? -grad : grad) + weight_decay * param;  exp_avg.lerp_(grad', 1 - beta1);
 *   exp_avg_sq = beta2 * exp_avg_sq + (1 - beta2) * grad'^2;  [amsgrad: max_exp_avg_sq = max(max_exp_avg_sq, exp_avg_sq)]
 *   param -= lr / (1 - beta1^step) * exp_avg / (sqrt(exp_avg_sq or its running max) / sqrt(1 - beta2^step) + eps)
 * on the optimizer's OWN state tensors (so optimizer.state_dict() stays what torch would have produced).
 * `step` is the count AFTER this update (>= 1); max_exp_avg_sq may be null (amsgrad off); all arrays [n] f32 on the device. */
int mg_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                 double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, int32_t maximize,
                 void* stream);
/* the same update, skipped entirely when *skip_flag != 0 (device int; may be null) */
int mg_adam_step_gated(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                       double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, int32_t maximize,
                       const int32_t* skip_flag, void* stream);

/* ---- end of a PPO epoch on the device (molgym/ppo.py:133-146: KL test, gradient norm, clip) --------------------------------
 * stats_accum[6] f64 = sum over the epoch's mini-batches of (share x statistics) (mg_cov_ppo_step); inv_num_minibatches = 1 / M.
 * rec[8] f64 <- {policy_loss, entropy_loss, vf_loss, total_loss, approx_kl, clip_fraction} means, the PRE-clip gradient norm,
 * and 1.0 if the update loop has stopped (this epoch's approx_kl > kl_limit, or an earlier epoch's was): the reference breaks
 * BEFORE the optimizer step in that case (ppo.py:139-141).  *stop_flag (device int, zero before the first epoch) latches; the
 * clip (grad *= min(1, max_norm / (norm + 1e-6)), max_norm > 0) is applied only while it is clear, and mg_adam_step_gated with
 * the same flag does nothing once it is set -- so the host may issue the next epoch without waiting for this one and read
 * `rec` late.  scratch: 1 float.                                                                                          */
int mg_ppo_epoch_end(int64_t n, float* grad, float max_norm, const double* stats_accum, double inv_num_minibatches,
                     double kl_limit, double* rec, int32_t* stop_flag, float* scratch, void* stream);

/* ---- ordered fold of per-mini-batch gradient rows (data-parallel training with the same bits at every world size) -----------
 * molgym_amd/ppo.py, ordered-DP mode: every mini-batch of an epoch writes its gradient and its statistics into a row of its own,
 * the rows of all ranks are gathered rank-major and added up here in GLOBAL mini-batch order, on every rank alike.
 *   row            [ n float32 gradient | 6 float64 statistics, raw bytes at byte n * 4 | pad ], row_stride_bytes apart;
 *                  `rows` is 16-byte aligned and row_stride_bytes a multiple of 16, at least n * 4 + 48 (else MG_EINVAL);
 *                  the statistics field needs no 8-byte alignment (n may be odd)
 *   rows           world blocks of per_rank rows each: [world][per_rank][row]; rank r's j-th mini-batch is global mini-batch
 *                  k = j * world + r, so global row k sits at rows[(k % world) * per_rank + k / world], k = 0 .. total - 1;
 *                  total <= world * per_rank; the remaining rows are padding and are never read
 *   grad_out[n]    <- (((+0.0f + row_0[i]) + row_1[i]) + ... + row_{total-1}[i]) in float32, strictly in k order
 *   stats_out[6]   <- the same fold of the statistics in float64 (may be NULL)
 * Both outputs are overwritten, not added to.  No atomics: the same rows give the same bits whatever `world` says about where
 * they sit.  Does not consult the mode switches.                                                                            */
int mg_fold_rows(int64_t n, int32_t world, int32_t per_rank, int32_t total, const void* rows, int64_t row_stride_bytes,
                 float* grad_out, double* stats_out, void* stream);

/* ---- test entry points of the grouped GEMM dispatchers (tests/test_gpu_gemm.py) --------------------------------------------
 * Every dense product of both agents goes through launch_gemm (forward Linears, channel mixes, input adjoints) and launch_dw
 * (weight gradients) in csrc/gemm_dispatch.inc, which choose among the kernel forms of csrc/gemm.inc by row count, alignment,
 * reduction length, output width and epilogue flags: a planner (plan_gemm / plan_gemm_dw, pure functions of the descriptors and the
 * switch table at the top of that file) chooses, a launch half carries the plan out.  mg_test_gemm / mg_test_gemm_dw translate a HOST array of group descriptors -- field for field the
 * dispatchers' own GemmG / GemmDwG, every pointer a DEVICE pointer -- and hand it to the dispatcher on `stream`, nothing else;
 * the weight-gradient call runs with deferral off (the launches are issued before it returns).  *forms_out_host (may be NULL)
 * receives the OR of the MG_FORM_* bits of the kernel forms the call launched, recursive splits included (more than 16 groups,
 * mixed column-tile classes of the VALU forms, runs of one weight-gradient class).
 *
 * mg_gemm_group:  Y[rows][N] = epilogue( sum_s X[s][rows][0..R) @ M[s][R][N] ), pitches ldx[s] / ldm / ldy, nseg in 1..5;
 *   epilogue in this order: + bias[col]; activation `relu` (0 none, 1 ReLU, 2 softplus - ln 2); posmask [rows][ld_mask] with
 *   mask_mode 1 (zero where mask <= 0) or 2 (times 1 - 0.5 exp(-mask)); * rowscale[row]; + resid [rows][ld_resid]; + the previous
 *   Y when `accumulate`.  Absent operands are NULL.
 * mg_gemm_dw_group:  dW[N][ldw] (first K columns) += dY[rows][N]^T @ X[rows][K];  db[N] += column sums of dY (db may be NULL);
 *   with X1 != NULL the reduction-side columns [ks1, ks2) come from X1 (from its column 0) and [ks2, K) from X2.
 *
 * Preconditions, as the kernels have them (the callers inside the library satisfy them by construction; nothing checks them):
 *   - M is zero padded to ldm, and ldm is N rounded up to its column tile (32 / 24 / 20 if one divides N, else 8): the VALU row
 *     forms load whole tiles of a weight row, the LDS-staged one as 16-byte quads;
 *   - the LDS-stationary row form (rows >= 16384, R >= 128, N <= 48) is only taken for N % 4 == 0, ldm % 4 == 0 and 16-byte
 *     aligned M / X; it zeroes its own pad rows R .. 64 ceil(R / 64) in LDS, none are read from memory;
 *   - a group with R % 4 != 0, ldx % 4 != 0 or an X that is not 16-byte aligned sends the whole call to the guarded forms;
 *   - the column forms take one segment and one R for all groups of a call; their vector stores need ldy % 4 == 0 and a
 *     16-byte aligned Y, otherwise (and with bias / activation / mask / resid) the scalar epilogue runs;
 *   - no form writes outside [rows][0..N): the pad columns [N, ldy) keep their contents;
 *   - dY may be over-read by fewer than 32 floats past its last row: the allocation needs that slack;
 *   - dW ACCUMULATES (atomics), and so does db;
 *   - ks1, ks2, ldx1, ldx2 of a concatenated X are multiples of 4 and X1 / X2 16-byte aligned (MG_EINVAL otherwise); a
 *     concatenated X needs the MFMA forms (N <= 128, MG_MFMA_DW != 0; MG_EINVAL otherwise);
 *   - the 8-byte / 16-byte X loads of the weight-gradient forms are only chosen when K, ldx and the alignment of X allow them
 *     for EVERY group of a run.
 * The shared-input and packed products (launch_sx / launch_pk) are tied to the build's channel counts and have no test entry. */
#define MG_GEMM_MAXSEG 5
typedef struct mg_gemm_group {
  const float* X[MG_GEMM_MAXSEG];
  const float* M[MG_GEMM_MAXSEG];
  int32_t ldx[MG_GEMM_MAXSEG];
  int32_t nseg;
  const float* bias;
  const float* rowscale;
  const float* posmask;
  const float* resid;
  float* Y;
  int32_t ldm, ldy, ld_mask, ld_resid, mask_mode;
  int32_t R, N, rows;
  int32_t relu;
  int32_t accumulate;
} mg_gemm_group;
typedef struct mg_gemm_dw_group {
  const float* dY;
  const float* X;
  const float* X1;
  const float* X2;
  int32_t ldx1, ldx2, ks1, ks2;
  float* dW;
  float* db;
  int32_t ldy, ldx, ldw;
  int32_t N, K, rows;
} mg_gemm_dw_group;
/* kernel forms (bit numbers; the binding lists the same names: molgym_amd/_lib.py::GEMM_FORMS).  Bits 3, 4, 7, 11 and 17
 * belonged to forms that were removed: they are retired and not to be reused.                                                  */
#define MG_FORM_ROWS_UNALIGNED 0   /* k_gemm_mfma_rows<NT, 4, false>: guarded loads                                   */
#define MG_FORM_ROWS_W4 1          /* k_gemm_mfma_rows<NT, 4>                                                         */
#define MG_FORM_ROWS_W16 2         /* k_gemm_mfma_rows_or<NT>: live tiles, 8 waves (MG_ROWS_W16_ONEROUND=0: rows<NT, 16>) */
#define MG_FORM_ROWS64_RT2 5       /* k_gemm_mfma_rows64<NT>: two 16-row tiles per wave                               */
#define MG_FORM_ROWS_WS 6          /* k_gemm_mfma_rows_ws<NT, LDW>: weights <= 80 KB of LDS                           */
#define MG_FORM_COLS_WS 8          /* k_gemm_mfma_cols_ws                                                             */
#define MG_FORM_MFMA_COLS_EXACT 9  /* k_gemm_mfma_cols<R / 4>: R = 8, 20, 24, 40                                      */
#define MG_FORM_MFMA_COLS_GENERIC 10 /* k_gemm_mfma_cols<8 | 16, false>                                               */
#define MG_FORM_ROWS_LDS 12        /* k_gemm_rows_lds<NT>                                                             */
#define MG_FORM_VALU_ROWS 13       /* k_gemm_rows<NT, V, WV>                                                          */
#define MG_FORM_DW4 16             /* k_gemm_mfma_dw4<NT8>: 16-byte X loads                                           */
#define MG_FORM_DW2 18             /* k_gemm_mfma_dw2: 8-byte X loads                                                 */
#define MG_FORM_DW 19              /* k_gemm_mfma_dw: dword X loads                                                   */
#define MG_FORM_VALU_DW 20         /* k_gemm_dw<NT>                                                                   */
int mg_test_gemm(const mg_gemm_group* groups_host, int32_t ng, uint64_t* forms_out_host, void* stream);
int mg_test_gemm_dw(const mg_gemm_dw_group* groups_host, int32_t ng, uint64_t* forms_out_host, void* stream);
/* mg_test_gemm as the forward callers inside the library issue it: mt_host[i] (may be NULL, as may mt_host itself) is a DEVICE
 * pointer to the transposed copy of group i's M[0], [N][ldmt_host[i]] with element [n][k] == M[0][k][n] for k < R (one segment only:
 * MG_EINVAL otherwise).  Only the one-round body of the rows_w16 form reads it, as 16-byte loads, when ldmt % 4 == 0, ldmt >= R and the
 * pointer is 16-byte aligned; every other form and every other group ignores it.  Its outputs are bit-identical with and without.
 * switches: as mg_test_gemm_plan (NULL: the process's table).                                                                  */
int mg_test_gemm_mt(const mg_gemm_group* groups_host, const void* const* mt_host, const int32_t* ldmt_host, int32_t ng,
                    const char* switches, uint64_t* forms_out_host, void* stream);
/* The same two calls, planner only: the same translation and the same walk (splits of more than 16 groups, one launch per group
 * for mixed column tiles, runs of one weight-gradient class), every launch counted instead of issued.  No device is touched and
 * no pointer dereferenced (the planner looks at their alignment only), so they run without a GPU.  *forms_out_host: the OR of the
 * MG_FORM_* bits mg_test_gemm / mg_test_gemm_dw would report; *launches_out_host: the number of kernel launches (either may be
 * NULL).  switches: NULL for the process's switch table (the environment at first use), else "NAME=VALUE NAME=VALUE" applied on
 * top of the DEFAULTS -- names as in the table of csrc/gemm_dispatch.inc, an unknown name is MG_EINVAL.  A call the dispatcher
 * refuses (concatenated input: misaligned, or without the MFMA forms) is MG_EINVAL here too.                                */
int mg_test_gemm_plan(const mg_gemm_group* groups_host, int32_t ng, const char* switches, uint64_t* forms_out_host,
                      int32_t* launches_out_host);
int mg_test_gemm_dw_plan(const mg_gemm_dw_group* groups_host, int32_t ng, const char* switches, uint64_t* forms_out_host,
                         int32_t* launches_out_host);
/* The DEFERRED weight-gradient path.  Inside a backward pass launch_dw parks its groups and flush_dw issues them together, bucketed
 * by class (N <= 32, <= 48, <= 128, the VALU tiles), at most 64 groups per launch.  mg_test_gemm_dw_flush parks `groups_host` that way
 * and flushes them on `stream`; *launches_out_host: the kernel launches issued.  mg_test_gemm_dw_flush_plan is its plan-only twin (as
 * mg_test_gemm_dw_plan: no device, no pointer dereferenced, `switches` on top of the defaults).  MG_EINVAL in deterministic mode.
 * The join (switch MG_DW_JOIN_WIDE, default 1; 0: every bucket its own launch): groups of 33..128 columns leave their bucket and run
 * in the launch of the N <= 32 bucket as 32-column n blocks of k_gemm_mfma_dw2<2> when (a) no ordered mode is bound, (b) that bucket is
 * non-empty, fits one launch with the joiners and plans the 8-byte form with the same rows per wave alone and joined, (c) the group
 * has an even K >= 32, even pitches and 8-byte aligned X / X1 / X2 (the others stay behind in their own launch), (d) the bucket the
 * group comes from plans fewer than 2048 workgroups on its own.  A joined launch reports BOTH MG_FORM_DW2 and MG_FORM_DW.  The
 * direct path (mg_test_gemm_dw, mg_test_gemm_dw_plan) never joins.                                                              */
int mg_test_gemm_dw_flush(const mg_gemm_dw_group* groups_host, int32_t ng, uint64_t* forms_out_host, int32_t* launches_out_host,
                          void* stream);
int mg_test_gemm_dw_flush_plan(const mg_gemm_dw_group* groups_host, int32_t ng, const char* switches, uint64_t* forms_out_host,
                               int32_t* launches_out_host);
/* The ordered weight-gradient form of deterministic mode, called directly (whatever the switch says).  Contract of
 * mg_gemm_dw_group: dW[N][ldw] (first K columns) += dY^T @ X, db[N] += column sums of dY, any N >= 1 and K >= 1, rows >= 1; no
 * atomics, nothing written outside [N][0..K), dY and X read inside [rows] only.  A group's rows are cut into chunks of
 * max(64, 64 ceil(rows / 4096)) rows -- a function of its `rows` alone, at most 64 chunks -- each chunk's partial product is stored
 * to scratch and the chunks are added to dW in index order by one thread per element, so a group's result does not depend on the
 * other groups of the call or on how the call is split into launches.  Groups of a call whose destinations are identical (dW,
 * db, N, K, ldw) are folded in list order: bit for bit what successive calls give; destinations are otherwise disjoint.
 * A concatenated input (X1 != NULL) is MG_EINVAL.  It has no MG_FORM_* bit.
 * scratch: 16-byte aligned device memory; mg_gemm_dw_ordered_scratch_bytes gives the size that lets the call run in the fewest
 * launches (32 groups at most per launch); any size that holds the largest single group works, MG_ENOMEM below that.       */
int mg_gemm_dw_ordered_scratch_bytes(const mg_gemm_dw_group* groups_host, int32_t ng, size_t* bytes_host);
int mg_test_gemm_dw_ordered(const mg_gemm_dw_group* groups_host, int32_t ng, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOLGYM_HIP_H */
