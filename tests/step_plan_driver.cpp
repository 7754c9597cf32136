// Stand-alone driver of csrc/ba_step_plan.hpp (tests/test_step_plan_host.py builds it with -fsanitize=address,undefined and runs it as
// a child process, once per switch setting): the rules that pick the point model's schedule, factorisation and back-substitution.
//   stdout: one JSON line per (cameras 1 .. 340, schur_impl 0 / 1, first step or not) with the FactorSetup and the StepPath of one
//           rank whose device probe of the pipeline succeeded, under the switches of the environment (StepSwitches::FromEnv) —
//           the Python test holds every line against tests/step_path_ref.py;
//   checks: what that reference cannot express — the invariants of keep_system_copy, communicators, first_staged, dec_step and a
//           small chip, the communicator rules of the pipeline, and the three stall transitions from every reachable state.
// A violated check ends the program with a non-zero status.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "ba_step_plan.hpp"

using namespace rsba;

static long g_checks = 0;
#define CHECK(cond)                                                                   \
  do {                                                                                \
    ++g_checks;                                                                       \
    if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s (C %d impl %d comm %d)\n", __FILE__, __LINE__, #cond, g_C, g_impl, (int)g_comm); exit(1); } \
  } while (0)
static int g_C = 0, g_impl = 0;
static bool g_comm = false;

static bool Same(const StepState& a, const StepState& b) {
  return a.pipelined == b.pipelined && a.pipelined_mg == b.pipelined_mg && a.pipe_serial == b.pipe_serial && a.pipeline_off == b.pipeline_off &&
         a.test_stall == b.test_stall && a.test_seq_stall_fired == b.test_seq_stall_fired && a.tiles_small == b.tiles_small && a.chol_wgs == b.chol_wgs &&
         a.chol_diag == b.chol_diag && a.border_cols == b.border_cols && a.tc_tiles == b.tc_tiles && a.has_tc_xs == b.has_tc_xs &&
         a.has_first_order == b.has_first_order && a.pipe_stalls == b.pipe_stalls && a.other_stalls == b.other_stalls &&
         a.pipe_check_resident == b.pipe_check_resident;
}

// The state UploadPoints leaves: the pipeline's device probes are taken to have succeeded (a loopback communicator: the
// multi-GPU pipeline too).
static StepState InitialState(int C, int impl, bool comm, int cus, const StepSwitches& sw, bool has_first_order, FactorSetup* setup) {
  StepState st;
  if (impl != 0) {
    const PipelineRule rule = PlanPipeline(C, comm, false, 1, true, sw);
    if (rule.armed) { st.pipe_serial = sw.pipeline == 2; st.test_stall = sw.test_stall; }
    st.pipelined = rule.eligible;
    st.pipelined_mg = rule.eligible && comm;
  }
  *setup = PlanFactorSetup(C, impl, comm, cus, sw);
  AdoptFactorSetup(st, *setup);
  st.has_first_order = has_first_order;
  return st;
}

static void CheckPath(const StepState& st, const StepSwitches& sw, int C, int impl, bool comm, bool first, bool keep) {
  const StepPath p = PlanStep(st, sw, C, impl, comm, first, keep);
  CHECK(p.fact >= kFactOneWg && p.fact <= kFactMultiLaunch && p.backsub >= kBacksubInKernel && p.backsub <= kBacksubChain && p.workgroups >= 1);
  CHECK(p.diag == (p.fact == kFactDiag || p.fact == kFactDiagBorder) && p.border == (p.fact == kFactDiagBorder));
  CHECK((p.backsub == kBacksubInKernel) == (p.fact <= kFactDiagBorder));
  // a caller's copies of the system: the sequential schedule, k_sys_build, the one-workgroup kernel up to 64 cameras
  if (keep) CHECK(!p.pipelined && !p.sys_fused && !p.diag);
  if (impl == 0 || st.pipeline_off) CHECK(!p.pipelined);
  if (!p.pipelined) CHECK(!p.mg && !p.serial && !p.first_staged && !p.check_resident && p.gate_skew == 0);
  if (p.pipelined) CHECK(6 * C <= RSBA_CHOL_MAXN && C > RSBA_TG && p.fact <= kFactDiagBorder);
  if (p.first_staged) CHECK(first && p.diag && !p.mg && st.has_first_order);
  if (p.mg) CHECK(comm && !p.allreduce && !p.border && !p.serial);
  if (p.dec_step) CHECK(p.use_proj);
  if (p.use_proj) CHECK(impl != 0 && C <= 256 && p.point_backsub == kPointBacksubProjective);
  CHECK(p.comm_tail == comm && (p.allreduce ? comm : true) && (p.tri_payload ? p.allreduce : true));
  if (p.border) CHECK(!comm && st.border_cols > 0 && st.border_cols < 6 * C);
  if (p.fact == kFactTilesSmall || p.fact == kFactTiled) CHECK(p.workgroups == st.tc_tiles && st.tc_tiles > 0);
  if (p.backsub == kBacksubChain) CHECK(st.has_tc_xs && st.tc_tiles > 0);
  if (p.sys_fused) CHECK(st.tc_tiles > 0);
  if (st.test_stall == 0) CHECK(p.gate_skew == 0 && p.solve_skew == 0 && !p.tiles_stall);
}

// The recoveries, from `st`: each leaves what the step's own code left before the rules moved into the plan.
static void CheckTransitions(const StepState& st0, const StepSwitches& sw, int C, int impl, bool comm, int depth) {
  for (bool first : {false, true}) for (bool keep : {false, true}) CheckPath(st0, sw, C, impl, comm, first, keep);
  if (depth == 0) return;
  {
    // tiled factorisation stalled: the multi-launch factorisation from now on, nothing else moves
    StepState st = st0, want = st0;
    OnTilesStalled(st);
    want.other_stalls += 1; want.tc_tiles = 0;
    CHECK(Same(st, want));
    const StepPath p = PlanStep(st, sw, C, impl, comm, false, false);
    CHECK(p.fact != kFactTilesSmall && p.fact != kFactTiled && p.backsub <= kBacksubOneWg && !p.sys_fused);
    CheckTransitions(st, sw, C, impl, comm, depth - 1);
  }
  {
    // multi-workgroup factorisation stalled: one workgroup; with a border, border off and the pipeline off for good
    StepState st = st0, want = st0;
    OnMultiWgStalled(st);
    want.test_seq_stall_fired = true; want.other_stalls += 1; want.chol_wgs = 1;
    if (st0.border_cols > 0) { want.border_cols = 0; want.pipeline_off = true; want.pipelined = false; want.pipelined_mg = false; }
    CHECK(Same(st, want));
    for (bool first : {false, true}) {
      const StepPath p = PlanStep(st, sw, C, impl, comm, first, false);
      CHECK(!p.diag && !p.border && !p.first_staged);
      if (st0.border_cols > 0) CHECK(!p.pipelined);
    }
    CheckTransitions(st, sw, C, impl, comm, depth - 1);
  }
  if (st0.pipelined) {
    // pipelined step stalled: a sequential repeat, the pipeline back while fewer than three stalls and not switched off
    StepState st = st0, want = st0;
    const bool was_mg = BeginSequentialRepeat(st);
    want.pipe_stalls += 1; want.pipelined = false; want.pipelined_mg = false;
    CHECK(Same(st, want) && was_mg == st0.pipelined_mg);
    CHECK(!PlanStep(st, sw, C, impl, comm, false, false).pipelined);
    CheckTransitions(st, sw, C, impl, comm, depth - 1);   // (what may happen to the repeat itself)
    StepState off = st;
    OnMultiWgStalled(off);                                // (the double fault: the repeat's factorisation stalls too)
    EndSequentialRepeat(st, was_mg);
    const bool back = want.pipe_stalls < 3 && (st0.test_stall == 0 || st0.test_stall == 4) && !st0.pipeline_off;
    if (back) { want.pipelined = true; want.pipelined_mg = st0.pipelined_mg; want.pipe_check_resident = true; }
    CHECK(Same(st, want));
    if (back) CHECK(PlanStep(st, sw, C, impl, comm, false, false).check_resident);
    CheckTransitions(st, sw, C, impl, comm, depth - 1);   // (twice, three times in a row)
    const bool off_for_good = off.pipeline_off;
    EndSequentialRepeat(off, was_mg);
    if (off_for_good) CHECK(!off.pipelined && !off.pipelined_mg);
  }
}

static void CheckStallClasses(const StepState& st, const StepSwitches& sw, int C, int impl, bool comm) {
  const StepPath p = PlanStep(st, sw, C, impl, comm, false, false);
  if (st.test_stall != 4) CHECK(ClassifyStall(st, p, false, false) == kNoStall);
  const StallKind k = ClassifyStall(st, p, true, false);
  if (p.pipelined) CHECK(k == kPipelineStalled && ClassifyStall(st, p, false, true) == kPipelineStalled);
  else if (st.tc_tiles > 0) CHECK(k == kTilesStalled);
  else if (st.chol_wgs > 1) CHECK(k == kMultiWgStalled);
  else CHECK(k == kNoStall);
  if (!p.pipelined) CHECK(ClassifyStall(st, p, false, true) == (st.test_stall == 4 && st.chol_wgs > 1 && st.pipe_stalls > 0 && !st.test_seq_stall_fired ? kMultiWgStalled : kNoStall));
}

static void CheckPipelineRules(const StepSwitches& sw0) {
  g_C = 40;
  StepSwitches sw = sw0;
  sw.pipeline = 1; sw.pipeline_mg = StepSwitches::kUnset; sw.hw_queues = 2;
  CHECK(PlanPipeline(40, false, false, 1, false, sw).eligible);
  CHECK(!PlanPipeline(16, false, false, 1, false, sw).eligible && !PlanPipeline(65, false, false, 1, false, sw).eligible && PlanPipeline(17, false, false, 1, false, sw).eligible &&
        PlanPipeline(64, false, false, 1, false, sw).eligible);
  CHECK(PlanPipeline(40, true, false, 4, true, sw).eligible && PlanPipeline(40, true, true, 1, true, sw).eligible);
  CHECK(!PlanPipeline(40, true, true, 2, true, sw).eligible);       // real RCCL, several ranks: opt-in
  CHECK(!PlanPipeline(40, true, false, 4, false, sw).eligible);     // a communicator that cannot have resident waiters
  CHECK(PipelineNeedsAgreement(true, sw) && !PipelineNeedsAgreement(false, sw));
  sw.pipeline_mg = 1;
  CHECK(PlanPipeline(40, true, true, 2, true, sw).eligible);
  sw.pipeline_mg = 0;
  CHECK(!PlanPipeline(40, true, false, 4, true, sw).eligible && PlanPipeline(40, false, false, 1, false, sw).eligible && !PipelineNeedsAgreement(true, sw));
  sw.pipeline_mg = StepSwitches::kUnset;
  for (int q : {0, 1, 2, 3, 4, 8}) {
    sw.hw_queues = q;
    const PipelineRule r = PlanPipeline(40, true, false, 2, true, sw);
    CHECK(r.eligible == (q != 3) && r.queue_note == (q == 3 ? 3 : (q == 1 || q == 2 || q == 8 ? 0 : 1)));
    CHECK(PlanPipeline(40, false, false, 1, false, sw).queue_note == 0);
  }
  sw.pipeline = 0;
  CHECK(!PlanPipeline(40, false, false, 1, false, sw).armed && !PlanPipeline(40, false, false, 1, false, sw).eligible && !PipelineNeedsAgreement(true, sw));
}

int main() {
  const StepSwitches sw = StepSwitches::FromEnv();
  CheckPipelineRules(sw);
  for (int C = 1; C <= 340; ++C) {
    for (int impl = 0; impl <= 1; ++impl) {
      g_C = C; g_impl = impl; g_comm = false;
      // ---- the lines the reference is held against: one rank, 256 CUs
      FactorSetup f;
      const StepState st = InitialState(C, impl, false, 256, sw, true, &f);
      for (int first = 0; first <= 1; ++first) {
        const StepPath p = PlanStep(st, sw, C, impl, false, first != 0, false);
        printf("{\"C\": %d, \"impl\": %d, \"first\": %d, \"setup\": {\"tiles_small\": %d, \"multi_wg\": %d, \"chol_wgs\": %d, \"chol_diag\": %d, \"border_cols\": %d, "
               "\"tc_np\": %d, \"tc_nrt\": %d, \"tc_tiles\": %d, \"tile_map\": %d, \"mc_flags\": %zu, \"mc_dg\": %zu, \"tc_flags\": %zu, \"tc_hand\": %zu, \"tc_xs\": %zu, \"tc_ys\": %zu}, "
               "\"path\": {\"pipelined\": %d, \"fact\": %d, \"workgroups\": %d, \"border_cols\": %d, \"tiles\": %d, \"backsub\": %d, \"sys_fused\": %d, "
               "\"serial\": %d, \"mg\": %d, \"first_staged\": %d, \"use_proj\": %d, \"point_backsub\": %d, \"dec_step\": %d, \"comm_tail\": %d, \"tri_payload\": %d}}\n",
               C, impl, first, (int)f.tiles_small, (int)f.multi_wg, f.chol_wgs, (int)f.chol_diag, f.border_cols, f.tc_np, f.tc_nrt, f.tc_tiles, (int)f.tile_map, f.mc_flags, f.mc_dg,
               f.tc_flags, f.tc_hand, f.tc_xs, f.tc_ys, p.pipelined, p.fact, p.workgroups, p.fact == kFactDiagBorder ? st.border_cols : 0,
               p.fact == kFactTilesSmall || p.fact == kFactTiled ? st.tc_tiles : 0, p.backsub, p.sys_fused, (int)p.serial, (int)p.mg, (int)p.first_staged, (int)p.use_proj,
               p.point_backsub, (int)p.dec_step, (int)p.comm_tail, (int)p.tri_payload);
      }
      // ---- what the reference cannot say
      for (bool comm : {false, true}) for (int cus : {256, 8}) for (bool first_order : {true, false}) for (int stall : {-1, 0, 1, 2, 3, 4}) {
        g_comm = comm;
        StepSwitches w = sw;
        if (stall >= 0) w.test_stall = stall;   // (-1: as the environment has it)
        FactorSetup fs;
        const StepState s0 = InitialState(C, impl, comm, cus, w, first_order, &fs);
        if (comm) CHECK(fs.border_cols == 0);   // a communicator never gets a border
        CHECK(fs.chol_wgs >= 1 && fs.chol_wgs <= 8 && (fs.chol_diag ? fs.chol_wgs >= 2 && fs.mc_dg != 0 : fs.chol_wgs == 1 && fs.mc_dg == 0) && (fs.border_cols > 0 ? fs.chol_diag : true));
        CHECK((fs.mc_flags != 0) == fs.multi_wg && (fs.tc_tiles > 0) == (fs.tc_flags != 0) && (fs.tc_tiles > 0) == (fs.tc_hand != 0) && (fs.tc_tiles > 0) == (fs.tc_xs != 0) &&
              (fs.tc_tiles > 0) == (fs.tc_ys != 0) && (fs.tile_map ? fs.tc_tiles > 0 : true));
        {
          // the resident tiles only where they all fit, two per CU
          const int m = (6 * C + 31) / 32 * 32, nrt = (m + 1 + 63) / 64, ntiles = nrt * (nrt + 1) / 2;
          if (ntiles > 2 * cus) CHECK(fs.tc_tiles == 0);
          else if (fs.tc_tiles > 0) CHECK(fs.tc_tiles == ntiles && fs.tc_nrt == nrt && fs.tc_np == m / 32 && fs.tc_flags == (size_t)fs.tc_np * (nrt + 2) + 1);
          if (6 * C <= RSBA_CHOL_MAXN && !fs.tiles_small) CHECK(fs.tc_tiles == 0);
        }
        CheckStallClasses(s0, w, C, impl, comm);
        CheckTransitions(s0, w, C, impl, comm, 3);
      }
    }
  }
  fprintf(stderr, "step plan driver: ok, %ld checks\n", g_checks);
  return 0;
}
