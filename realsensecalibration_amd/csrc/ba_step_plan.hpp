// Host-side planning of the point model's reduced-system path: which schedule, factorisation and back-substitution a step
// runs, what UploadPoints has to allocate for them, and what a stalled step leaves behind.  Plain C++, header-only: nothing
// here touches the GPU, and the environment is read in one place (StepSwitches::FromEnv, once per solver), so the whole unit
// runs under the host sanitizers (tests/step_plan_driver.cpp).  ba_solver.hip allocates from a FactorSetup and launches from a
// StepPath; LDS byte counts and grids that depend on the kernel headers stay with the launches.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdlib>
#include <string>

#include "ba_schur_plan.hpp"   // RSBA_TG, RSBA_CHOL_MAXN, RSBA_PB, RSBA_CT, RSBA_BSM_BPG, MultiCholPadded, kTileHandDoubles

namespace rsba {

// Every switch that chooses a path or a diagnostic of the point model's set-up and step.
struct StepSwitches {
  static constexpr int kUnset = INT_MIN;
  int pipeline = 1;             // RSBA_PIPELINE: 0 the sequential schedule, 2 the pipelined schedule's kernels one after the other, 3 the one-bit CU mask
  int pipeline_mg = kUnset;     // RSBA_PIPELINE_MG: 0 the sequential multi-GPU schedule, 1 the pipelined one over real RCCL with several ranks too
  int test_stall = 0;           // RSBA_TEST_STALL (>= 1 when set): armed by SetupPipeline, StepState::test_stall
  bool tiles_small = false;     // RSBA_TILES_SMALL=1: the persistent tiled factorisation for 17 .. 64 cameras, sequential schedule
  bool fused_lin = true;        // RSBA_FUSED_LIN=0: every step runs the full point pass (the round-1 schedule)
  int chol_wgs = kUnset;        // RSBA_CHOL_WGS: workgroups of the diagonal-chain factorisation (up to 8)
  bool border = true;           // RSBA_BORDER=0: every camera group through the diagonal-chain kernel
  bool chol_tiles = true;       // RSBA_CHOL_TILES=0: the multi-launch factorisation above 64 cameras
  bool tile_order = true;       // RSBA_TILE_ORDER=0: row by row (the pairing of tiles on shared CUs left to chance)
  int tri_payload = kUnset;     // RSBA_TRI_PAYLOAD: 1 / 0 forces / disables the triangular all-reduce payload
  bool first_staged = true;     // RSBA_FIRST_STAGED=0: a run's first step waits for all stages
  bool sys_fused = true;        // RSBA_SYS_FUSED=0: k_sys_build in front of the resident tiles too
  int backsub_multi = 2;        // RSBA_BACKSUB_MULTI: 2 k_backsub_chain, 1 k_backsub_multi, 0 k_chol_finish
  bool backsub_proj = true;     // RSBA_BACKSUB_PROJ=0: the form that reads the camera constants themselves
  bool decided_damp = true;     // RSBA_DECIDED_DAMP=0: the host launches the damping kernel once it has decided itself
  int resident_spare = 12;      // RSBA_RESIDENT_SPARE: workgroup slots a resident Schur launch leaves free (RSBA_RESIDENT builds)
  int trace = kUnset;           // RSBA_TRACE: 1 step stamps, 2 Schur block timeline, 3 ring of the last steps, 4 back-substitution workgroups
  bool mc_trace = false;        // RSBA_MC_TRACE: stamps of the multi-workgroup / tiled factorisation
  bool has_trace_file = false;  // RSBA_TRACE_FILE: where the timelines of RSBA_TRACE=2 / 4 go
  std::string trace_file;
  bool debug = false;           // RSBA_DEBUG: set-up notes on stderr
  int hw_queues = 0;            // GPU_MAX_HW_QUEUES as the process was started with it (0: unset); read only

  static StepSwitches FromEnv() {
    StepSwitches w;
    auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    auto not_zero = [&](const char* name) { return num(name, 1) != 0; };
    w.pipeline = num("RSBA_PIPELINE", 1);
    w.pipeline_mg = num("RSBA_PIPELINE_MG", kUnset);
    w.test_stall = getenv("RSBA_TEST_STALL") ? std::max(1, num("RSBA_TEST_STALL", 0)) : 0;
    w.tiles_small = num("RSBA_TILES_SMALL", 0) != 0;
    w.fused_lin = not_zero("RSBA_FUSED_LIN");
    w.chol_wgs = num("RSBA_CHOL_WGS", kUnset);
    w.border = not_zero("RSBA_BORDER");
    w.chol_tiles = not_zero("RSBA_CHOL_TILES");
    w.tile_order = not_zero("RSBA_TILE_ORDER");
    w.tri_payload = num("RSBA_TRI_PAYLOAD", kUnset);
    w.first_staged = not_zero("RSBA_FIRST_STAGED");
    w.sys_fused = not_zero("RSBA_SYS_FUSED");
    w.backsub_multi = num("RSBA_BACKSUB_MULTI", 2);
    w.backsub_proj = not_zero("RSBA_BACKSUB_PROJ");
    w.decided_damp = not_zero("RSBA_DECIDED_DAMP");
    w.resident_spare = num("RSBA_RESIDENT_SPARE", 12);
    w.trace = num("RSBA_TRACE", kUnset);
    w.mc_trace = getenv("RSBA_MC_TRACE") != nullptr;
    if (const char* f = getenv("RSBA_TRACE_FILE")) { w.has_trace_file = true; w.trace_file = f; }
    w.debug = getenv("RSBA_DEBUG") != nullptr;
    w.hw_queues = num("GPU_MAX_HW_QUEUES", 0);
    return w;
  }
};

// ------------------------------------------------------------------------------------------------
// Set-up: the factorisation's geometry and buffers (UploadPoints allocates them)
// ------------------------------------------------------------------------------------------------
struct FactorSetup {
  bool tiles_small = false;   // RSBA_TILES_SMALL=1 (opt-in, round 5): the persistent TILED factorisation + chain back-substitution (ba_cholesky_tiles.hpp)
                              // for 17 .. 64 cameras in the SEQUENTIAL schedule: 130 + 26 us against the diagonal-chain kernel's 170 at 64 cameras
                              // (0.436 against 0.449 ms per step).  Opt-in because its roundings are not the pipelined schedule's kernel's: the two
                              // schedules — and a step repeated sequentially after a stall — would no longer add the same bits.
  bool multi_wg = false;      // the diagonal-chain kernel's flags and attributes are wanted (32 .. 64 cameras, tiled Schur kernel, more than one workgroup asked for)
  int chol_wgs = 1;           // > 1: the reduced system is factored by this many workgroups (ba_cholesky_multi.hpp)
  bool chol_diag = false;     // ... with the diagonal chain in workgroup 0 (ba_cholesky_diag.hpp)
  int border_cols = 0;        // > 0 (RSBA_BORDER=1; 33 .. 64 cameras, no communicator): the diagonal-chain kernel factors the leading 96 B columns and one more
                              // workgroup forms the last camera group as their border (ba_cholesky_border.hpp); both schedules, so that they add the same bits
  int tc_np = 0, tc_nrt = 0, tc_tiles = 0;   // persistent tiled factorisation: panels, tile rows, tiles (0 tiles: the multi-launch path)
  bool tile_map = false;      // ... with TileOrder's placement of its workgroups
  // element counts (0: not allocated)
  size_t mc_flags = 0;        // ints: tdone[16] | strip_ready[16] | wg_done[8] | error
  size_t mc_dg = 0;           // doubles: look-ahead sums | blocks as handed over
  size_t tc_flags = 0;        // ints: tdone | xdone | error | xdone of the back-substitution
  size_t tc_hand = 0;         // doubles: the diagonal chain's hand-over buffers, two sets
  size_t tc_xs = 0, tc_ys = 0;   // doubles: k_backsub_chain's hand-overs, two sets each: x and the helpers' slices of y
};

inline FactorSetup PlanFactorSetup(int C, int schur_impl, bool has_comm, int cus, const StepSwitches& sw) {
  FactorSetup f;
  const int nc = 6 * C;
  f.tiles_small = sw.tiles_small && nc <= RSBA_CHOL_MAXN && C > RSBA_TG;
  // several workgroups for the reduced system: 32 to 64 cameras (padded to whole 32-wide panels), full symmetric S
  // (the diagonal-chain kernel, one workgroup for the diagonal + five for the rows below by default: 0.469 against 0.474 ms per
  //  LM iteration with three row workgroups — fewer blocks per workgroup, more K slices per block; up to 8)
  // (the last camera group as a border — three camera groups or more, the tiled Schur kernel, one rank; RSBA_BORDER=0: every camera group
  //  through the diagonal-chain kernel — leaves that kernel nine panels instead of twelve at 64 cameras: ONE diagonal and THREE row
  //  workgroups then (round 6; six alternating runs on one box: 0.3452 - 0.3470 ms per step against 0.3489 - 0.3513 with five row
  //  workgroups, the driver's twenty-step command 0.3485 against 0.3527; 5: 0.3478 - 0.3483, 7 / 8: 0.351 - 0.353 — every workgroup of
  //  the factorisation holds a CU's whole LDS for the length of the step, and the row workgroups' traffic shares the Schur kernel's paths))
  const int ngroups_c = (C + RSBA_TG - 1) / RSBA_TG;
  const bool border_ok = sw.border && !has_comm && ngroups_c >= 3;
  const int want = sw.chol_wgs != StepSwitches::kUnset ? sw.chol_wgs : (border_ok ? 3 : 6);
  if (want > 1 && schur_impl != 0 && nc >= 6 * RSBA_PB && nc <= RSBA_CHOL_MAXN) {
    f.multi_wg = true;
    f.chol_wgs = std::min(want, 8);
    f.mc_flags = 64;
    // a row workgroup of the diagonal-chain kernel keeps the look-ahead sums of at most four blocks
    const int np_d = MultiCholPadded(nc) / RSBA_PB;
    const int np_rule = border_ok ? 3 * (ngroups_c - 1) : np_d;   // panels of the system the diagonal-chain kernel factors (the border's workgroup has the rest)
    f.chol_diag = f.chol_wgs >= 2 && (np_rule - 2 + f.chol_wgs - 2) / (f.chol_wgs - 1) <= 4;
    if (!f.chol_diag) f.chol_wgs = 1;   // (more blocks per row workgroup than the diagonal-chain kernel keeps sums for: one workgroup)
    if (f.chol_diag) f.mc_dg = (size_t)2 * (np_d + 1) * 1024;
    // the last camera group as a border: three camera groups or more, the tiled Schur kernel, one rank
    if (border_ok && f.chol_diag) f.border_cols = 6 * RSBA_TG * (ngroups_c - 1);
  }
  // more than 64 cameras: one resident workgroup per 64 x 64 tile, if they all fit on the chip at once (two per CU)
  if ((nc > RSBA_CHOL_MAXN || f.tiles_small) && sw.chol_tiles) {
    const int m = MultiCholPadded(nc), nrt = (m + 1 + 63) / 64, ntiles = nrt * (nrt + 1) / 2;
    if (ntiles <= 2 * cus) {
      f.tc_np = m / RSBA_PB; f.tc_nrt = nrt; f.tc_tiles = ntiles;
      f.tc_flags = (size_t)f.tc_np * (nrt + 2) + 1;
      f.tile_map = sw.tile_order;
      f.tc_hand = (size_t)2 * nrt * kTileHandDoubles;
      const int H = (f.tc_np + 2) / 3;
      f.tc_xs = (size_t)2 * m; f.tc_ys = (size_t)2 * H * 96;
    }
  }
  return f;
}

// triangular all-reduce payload: by default where bytes bound the collective (more than 64 cameras), RSBA_TRI_PAYLOAD=1 / 0 forces / disables it
inline bool WantsTriPayload(int C, bool has_comm, const StepSwitches& sw) {
  return has_comm && (sw.tri_payload != StepSwitches::kUnset ? sw.tri_payload != 0 : 6 * C > RSBA_CHOL_MAXN);
}

// The part of the pipelined schedule's eligibility that needs no device (SetupPipeline creates the streams and probes them).
struct PipelineRule {
  bool armed = false;      // RSBA_PIPELINE != 0: the test hooks are read, RSBA_PIPELINE=2 gets its events
  bool eligible = false;   // worth creating and probing the side streams
  int queue_note = 0;      // with a communicator: 3 the pool of three hardware queues (sequential schedule), 1 a pool that starts the kernels late
};
inline PipelineRule PlanPipeline(int C, bool has_comm, bool comm_is_rccl, int nranks, bool allows_resident_waiters, const StepSwitches& sw) {
  PipelineRule r;
  r.armed = sw.pipeline != 0;
  if (!r.armed) return r;
  if (has_comm) {
    // Multi-GPU pipeline: ON by default with a communicator (RSBA_PIPELINE_MG=0: the sequential multi-GPU schedule).
    if (sw.pipeline_mg == 0) return r;
    // Round 5 (ADVICE, medium): over REAL RCCL with more than one rank the pipelined schedule is opt-in (RSBA_PIPELINE_MG=1) until
    // an N >= 2 run on hardware is on record — RCCL's own kernels then need CUs and hardware queues beside the resident waiters
    // (k_wait_stage, the gated factorisation), and every stall costs ten stall budgets before the step is repeated.  Loopback and
    // shared-memory groups and 1-rank communicators, where it has run thousands of steps, keep it as their default.
    if (comm_is_rccl && nranks > 1 && sw.pipeline_mg != 1) return r;
    if (!allows_resident_waiters) return r;
    // The one setting it cannot live with is a pool of THREE hardware queues (the waiting kernels land behind each other: every
    // step times out): then the sequential schedule is used, and the library says so once.
    if (sw.hw_queues == 3) { r.queue_note = 3; return r; }
    if (sw.hw_queues != 8 && sw.hw_queues != 1 && sw.hw_queues != 2) r.queue_note = 1;
  }
  if (C <= RSBA_TG) return r;   // one camera group: nothing to overlap
  // More than 64 cameras: the sequential schedule.  (A persistent tiled factorisation gated beside the Schur kernel was slower
  // than it: one resident workgroup per 64 x 64 tile leaves the elimination too few workgroup slots — HISTORY.md, round 4.)
  if (6 * C > RSBA_CHOL_MAXN) return r;
  r.eligible = true;
  return r;
}

// Multi-GPU: the pipelined schedule issues other collectives than the sequential one, so the ranks have to agree — whenever
// some rank of the group could pipeline at all.
inline bool PipelineNeedsAgreement(bool has_comm, const StepSwitches& sw) { return has_comm && sw.pipeline != 0 && sw.pipeline_mg != 0; }

// ------------------------------------------------------------------------------------------------
// The step
// ------------------------------------------------------------------------------------------------
// What a step's rules read of the solver, and what the stall recoveries write.
struct StepState {
  // Pipelined solve (single GPU, 17..64 cameras): the Cholesky is launched FIRST, on its own hardware queue, and waits inside the
  // kernel for ready flags; the pair kernel (on the main stream) publishes each camera group's columns as its last workgroups
  // reduce them, the self tiles are the first blocks of the same launch.
  bool pipelined = false;
  // Multi-GPU pipeline: the stage flags the Cholesky waits on are published on the communication stream, each after the
  // all-reduce of that stage's row slab of S (k_wait_stage / k_set_flag, ba_schur_tiled.hpp)
  bool pipelined_mg = false;
  bool pipe_serial = false;   // RSBA_PIPELINE=2: the pipelined schedule's kernels launched one after the other (counter collection)
  bool pipeline_off = false;  // the one-workgroup fallback was taken with a bordered work list (or any other state the pipelined schedule's
                              // gates do not describe): the solver stays sequential for good
  int test_stall = 0;         // RSBA_TEST_STALL=1: the Cholesky waits for a tag nobody publishes, =2: the back-substitution does,
                              // =3: a diagonal tile of the persistent tiled factorisation waits for a hand-over nobody writes
                              // (both exercise the fallback to the sequential schedule); =4: the DOUBLE fault — the first pipelined
                              // step stalls as with 1, and its sequential repeat reports a stalled multi-workgroup factorisation once
                              // (the one-workgroup fallback; later steps are NOT forced sequential, so the re-enable logic is what runs)
  bool test_seq_stall_fired = false;
  bool tiles_small = false;   // FactorSetup
  int chol_wgs = 1;
  bool chol_diag = false;
  int border_cols = 0;
  int tc_tiles = 0;
  bool has_tc_xs = false;     // k_backsub_chain's hand-over buffers exist
  bool has_first_order = false;   // the Schur plan holds a launch order for a run's first step (SchurPlan::border_first)
  // pipelined schedule: steps that timed out (the step is repeated sequentially; the third time-out ends the pipelined
  // schedule for this solver), and "the next pipelined step waits until the factorisation is resident" (first step of a
  // run, first step after a time-out)
  int pipe_stalls = 0;
  int other_stalls = 0;       // stalls of the multi-workgroup / tiled factorisation in the sequential schedule (each is a permanent fallback)
  bool pipe_check_resident = false;
};

inline void AdoptFactorSetup(StepState& st, const FactorSetup& f) {
  st.tiles_small = f.tiles_small; st.chol_wgs = f.chol_wgs; st.chol_diag = f.chol_diag; st.border_cols = f.border_cols;
  st.tc_tiles = f.tc_tiles; st.has_tc_xs = f.tc_xs != 0;
}

// bytes of LDS per camera of the LDS-staged back-substitution: both tables of camera constants and the camera step
// (ba_solver.hip asserts that it equals (2 RSBA_CC_LDS + 6) doubles)
constexpr int kBacksubLdsBytesPerCamera = 576;

enum Factorisation { kFactOneWg = 0, kFactDiag = 1, kFactDiagBorder = 2, kFactTilesSmall = 3, kFactTiled = 4, kFactMultiLaunch = 5 };
enum CameraBacksub { kBacksubInKernel = 0, kBacksubOneWg = 1, kBacksubMulti = 2, kBacksubChain = 3 };
enum PointBacksubForm { kPointBacksubProjective = 0, kPointBacksubLdsStaged = 1, kPointBacksubPlain = 2 };

// Everything a step branches on.  rsba_points_solve_stage reports pipelined, fact, workgroups, backsub and sys_fused of the
// last step (a step repeated after a stall overwrites it).
struct StepPath {
  int pipelined = 0;          // the pipelined schedule (1), the sequential one (0)
  bool serial = false;        // ... its kernels one after the other (RSBA_PIPELINE=2)
  bool mg = false;            // ... gated on the communication stream's stage flags
  bool first_staged = false;  // ... a run's first step gated stage by stage too (the Schur kernel runs every self tile first)
  bool check_resident = false;   // ... the host waits until the factorisation is resident before it launches the Schur kernel
  int gate_skew = 0;          // test hooks: added to the tag the factorisation's gates / the back-substitution's wait look for
  int solve_skew = 0;
  bool tiles_stall = false;   // test hook: a diagonal tile looks for its hand-over in the set nobody writes
  int fact = kFactOneWg;      // Factorisation
  bool diag = false;          // k_reduced_system_solve_diag (fact 1 or 2), else up to 64 cameras k_reduced_system_solve
  bool border = false;        // ... with the border's workgroup as the launch's last
  int workgroups = 1;         // of the factorisation (multi-launch: of its first panel's launch)
  int backsub = kBacksubInKernel;   // CameraBacksub
  int sys_fused = 0;          // the resident tiles build their entries of the system themselves (no k_sys_build)
  bool allreduce = false;     // the all-reduce of the whole reduced system behind the Schur kernel (a communicator, not the multi-GPU pipeline)
  bool tri_payload = false;   // ... as lower triangle + vectors
  bool fused_lin = false;     // the point back-substitution keeps the candidate's linearisation
  bool use_proj = false;      // k_backsub_candidate_proj
  int point_backsub = kPointBacksubPlain;   // PointBacksubForm
  bool comm_tail = false;     // the candidate's sums go through an all-reduce, k_publish_result posts the result
  bool dec_step = false;      // the device takes the step's decision and the next step's damping kernel is queued on it
};

inline StepPath PlanStep(const StepState& st, const StepSwitches& sw, int C, int schur_impl, bool has_comm, bool first, bool keep_system_copy) {
  StepPath p;
  const int n = 6 * C;
  const bool pipe = st.pipelined && schur_impl != 0 && !keep_system_copy;
  const bool diag_ok = st.chol_wgs > 1 && st.chol_diag;
  p.pipelined = pipe ? 1 : 0;
  if (pipe) {
    p.mg = st.pipelined_mg;
    p.serial = st.pipe_serial && !p.mg;
    // the first step of a run gated stage by stage too (diagonal-workgroup factorisation only): the Schur kernel runs every
    // self tile first and publishes ready[9] when all cameras' diag U are written (RSBA_FIRST_STAGED=0: wait for all stages)
    p.first_staged = first && sw.first_staged && st.has_first_order && diag_ok && !p.mg;
    p.check_resident = first || st.pipe_check_resident;
    p.gate_skew = (st.test_stall == 1 || (st.test_stall == 4 && st.pipe_stalls == 0)) ? 1 : 0;
    p.diag = diag_ok;
    p.border = p.diag && st.border_cols > 0 && !p.mg;
    p.fact = p.diag ? (p.border ? kFactDiagBorder : kFactDiag) : kFactOneWg;
    p.workgroups = p.diag ? st.chol_wgs + (p.border ? 1 : 0) : 1;
  } else if (n <= RSBA_CHOL_MAXN && !(st.tiles_small && st.tc_tiles > 0 && !keep_system_copy)) {
    p.diag = diag_ok && !keep_system_copy;
    p.border = p.diag && st.border_cols > 0;
    p.fact = p.diag ? (p.border ? kFactDiagBorder : kFactDiag) : kFactOneWg;
    p.workgroups = p.diag ? st.chol_wgs + (p.border ? 1 : 0) : 1;
  } else {
    // more than 64 cameras (or RSBA_TILES_SMALL): the resident tiles build their entries of the system themselves
    // (TileSysSource); k_sys_build only where its output is wanted for itself (the copies of the system a caller asked for) or
    // the multi-launch factorisation reads it
    p.sys_fused = st.tc_tiles > 0 && !keep_system_copy && sw.sys_fused ? 1 : 0;
    if (st.tc_tiles > 0) {
      p.fact = n <= RSBA_CHOL_MAXN ? kFactTilesSmall : kFactTiled;
      p.workgroups = st.tc_tiles;
      p.tiles_stall = st.test_stall == 3;
    } else {
      // right-looking factorisation over the whole chip, one launch per 32-wide panel
      const int nrt = (n + 1 - std::min(RSBA_PB, n) + RSBA_CT - 1) / RSBA_CT;
      p.fact = kFactMultiLaunch;
      p.workgroups = nrt * (nrt + 1) / 2;
    }
    // RSBA_BACKSUB_MULTI: 2 (default) the chain in one workgroup with helpers for the far strips (k_backsub_chain), 1 the chain
    // passed from owner to owner (k_backsub_multi, round 2), 0 one workgroup for everything (k_chol_finish)
    if (st.tc_tiles > 0 && sw.backsub_multi >= 2 && st.has_tc_xs) p.backsub = kBacksubChain;
    else if (st.tc_tiles > 0 && sw.backsub_multi >= 1) p.backsub = kBacksubMulti;
    else p.backsub = kBacksubOneWg;
  }
  p.solve_skew = (st.test_stall && (st.test_stall != 4 || st.pipe_stalls == 0)) ? st.test_stall * st.test_stall : 0;
  p.allreduce = has_comm && !(pipe && st.pipelined_mg);
  p.tri_payload = p.allreduce && WantsTriPayload(C, has_comm, sw);
  // single GPU: the back-substitution's last workgroup finishes the step (sums, result block, post to the host); with a
  // communicator the projective kernel's last workgroup leaves the rank's sums for the all-reduce, the other kernels their
  // per-block sums for k_finish_candidate
  // (RSBA_BACKSUB_PROJ=0: the form that reads the camera constants themselves, for comparison)
  p.fused_lin = schur_impl != 0 && sw.fused_lin;
  p.use_proj = p.fused_lin && sw.backsub_proj && C <= 256;
  p.point_backsub = p.use_proj ? kPointBacksubProjective
                               : ((size_t)C * kBacksubLdsBytesPerCamera <= 60 * 1024 ? kPointBacksubLdsStaged : kPointBacksubPlain);
  p.comm_tail = has_comm;
  // the workgroup that completes the result block takes the step's decision as well (RSBA_DECIDED_DAMP=0: the host launches the
  // damping kernel once it has decided itself)
  p.dec_step = p.use_proj && sw.decided_damp;
  return p;
}

// ------------------------------------------------------------------------------------------------
// Stalls: which of the step's in-kernel waits gave up, and the state the recovery leaves (the step is then repeated)
// ------------------------------------------------------------------------------------------------
enum StallKind { kNoStall = 0, kTilesStalled, kMultiWgStalled, kPipelineStalled };

inline StallKind ClassifyStall(const StepState& st, const StepPath& p, bool res_stall, bool wait_timeout) {
  if (!p.pipelined && st.tc_tiles > 0 && res_stall) return kTilesStalled;
  if (!p.pipelined && st.chol_wgs > 1 && (res_stall || (st.test_stall == 4 && st.pipe_stalls > 0 && !st.test_seq_stall_fired))) return kMultiWgStalled;
  if (p.pipelined && (res_stall || wait_timeout)) return kPipelineStalled;
  return kNoStall;
}

// persistent tiled Cholesky stalled: the multi-launch factorisation
inline void OnTilesStalled(StepState& st) { ++st.other_stalls; st.tc_tiles = 0; }

// the workgroups of the factorisation did not run side by side (cannot happen on an idle stream): one workgroup then
inline void OnMultiWgStalled(StepState& st) {
  st.test_seq_stall_fired = true;
  ++st.other_stalls;
  st.chol_wgs = 1;
  if (st.border_cols > 0) {
    // The Schur work list was built for the border (2 Bg + 1 stages, permuted: stage g holds the leading tiles only, tile (g, Bg) is
    // stage Bg + g, the border's own tile stage 2 Bg).  The one-workgroup factorisation's gates read ready[1 + g] as "all columns of
    // camera group g": pipelined again it would factor panels whose border rows are still being accumulated, silently.  No border,
    // and no pipelined schedule for this solver any more (a kernel boundary needs no stages).
    st.border_cols = 0;
    st.pipeline_off = true;
    st.pipelined = false; st.pipelined_mg = false;
  }
}

// A pipelined step stalled: the repeat runs sequentially; a solver that has timed out three times stays there.
inline bool PipelineRecovers(const StepState& st) { return st.pipe_stalls < 3 && (!st.test_stall || st.test_stall == 4) && !st.pipeline_off; }
// before the repeat; returns whether the schedule was the multi-GPU one
inline bool BeginSequentialRepeat(StepState& st) {
  ++st.pipe_stalls;
  const bool was_mg = st.pipelined_mg;
  st.pipelined = false; st.pipelined_mg = false;
  return was_mg;
}
// after it (the repeat may have switched the pipeline off for good)
inline void EndSequentialRepeat(StepState& st, bool was_mg) {
  if (PipelineRecovers(st)) { st.pipelined = true; st.pipelined_mg = was_mg; st.pipe_check_resident = true; }
}

}  // namespace rsba
