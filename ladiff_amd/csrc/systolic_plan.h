// The plan of the persistent denoiser loop (systolic.hip): the one description that the host planner (systolic_plan.hip) and the
// device code (systolic.hip) share - the plan constants, the stage table's and the block list's records, the workspace carve and the
// planner's entry points.  Plain C++17: no device code and no HIP header, so that the planner builds and runs without a GPU
// (tests/planner_check.cpp); and nothing here depends on a build variant's defines (the diagnostic builds recompile systolic.hip only).
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "weights.h"

namespace ladiff {

constexpr int NSLICE = 8;                 // hidden slices of the two MLPs (128 columns each)
constexpr int HS = FF / NSLICE;           // 128
constexpr int NRED = 3;                   // workgroups per layer of each of the two reduce stages (how they share the work: red_parts())
constexpr int NTAIL = 4;                  // tail workgroups (block b belongs to tail b % NTAIL)
constexpr int FLAG_SLOTS = 16;
// The eight partial planes of a layer's two K-split matrices (LIN -> RED2, FFN -> STYL) are RINGS of PRING block slots, not NB:
// with a buffer set per layer (sys_layout) they would otherwise be most of a working set larger than the 256 MiB memory-side
// cache.  A producer may therefore run at most PRING blocks ahead of its consumer: every PRING / 2 blocks it waits for the
// consumer's flag of the block PRING / 2 back (MlpRole::backpressure; the stages visit their blocks in order).  The slot of
// block b of local step s is (s NB + b) % PRING: blocks are counted THROUGH the steps, so that the reuse distance is PRING
// blocks at the wrap from one step to the next as well.
constexpr int PRING = 16;
// What the one-bit tag of a ring slot needs from these constants (the invariant in the header of systolic.hip).  A producer looks back
// every PRING / 2 blocks, at the consumer's block PRING / 2 back and - where the consumer is MAX_BP_BLOCKS groups on alternating
// blocks - at the blocks just before it: the look-back must be a whole number of blocks, and every block it looks at must lie
// inside the ring's previous half, so that "the consumer has finished them" covers exactly the slots the next PRING / 2 blocks overwrite.
constexpr int MAX_BP_BLOCKS = 2;            // consecutive blocks that make "all consumers" (Stage::bp_blocks <= this: red_plan's styl_groups)
static_assert(PRING >= 2 && PRING % 2 == 0, "the back-pressure look-back is PRING / 2 blocks");
static_assert(MAX_BP_BLOCKS <= PRING / 2, "every block a producer looks back at must be in the half ring it is about to leave alone");
constexpr int SMALL_LAUNCH_BLOCKS = 60;     // launches up to this many blocks: LIN / FFN rest after every block (sys_launch_policy)
constexpr int LOOK_AHEAD_BLOCKS = 72;       // launches from this many blocks look ahead (systolic.hip, `settle`): 58 blocks (128 prompts of mixed lengths) lose with it, 86 win
constexpr int FLAG_STRIDE = 32;             // words between the flags of two producers: every flag on a 128-byte line of its own
constexpr int SYS_LDS_BYTES = 100 * 1024;   // > 80 KiB: one workgroup per CU, so the <= 256 workgroups sit on distinct CUs
constexpr int GROUPS_PER_LAYER = 7;
enum Group : int { G_XIN = 0, G_ATT = 1, G_X1 = 2, G_PC = 3, G_X2 = 4, G_PE = 5, G_XO = 6 };
enum Role : int { R_QKV = 0, R_OUT = 1, R_LIN = 2, R_RED2 = 3, R_FFN = 4, R_STYL = 5, R_SKIP = 6, R_TAIL = 7 };

struct Stage {                            // one per workgroup
    int role, layer, slice, act;
    int wait_group, wait_n, out_group, out_slot;
    int blk0, blkstride;                  // the blocks this workgroup visits: blk0, blk0 + blkstride, ...
    // A flag with many consumer workgroups is REPLICATED, one 128-byte line per consumer: the producer raises out_rep flags (slots
    // out_slot + i out_rep_stride) with one store instruction, a consumer polls wait_n slots from wait_slot0.  Sixty-four waves
    // polling one line made every poll of that line slow - and those were the inputs of the two busiest stage types (LIN, FFN).
    int wait_slot0, out_rep, out_rep_stride;
    // XCD placement (sys_place_stages): workgroup i runs on XCD i % 8 and each XCD has an L2 of its own.  out_local = every reader
    // of this stage's output (rows and flags) sits on the SAME XCD: the stage then stores plainly - the rows stay in that L2, the
    // store is acknowledged by the L2 instead of the memory side (a hop of 0.5 us instead of 0.9 - 1.2 us,
    // scripts/ubench_xcd_handoff.hip) - otherwise it writes through (sc1).  Loads are sc1 either way: they are served by the
    // reader's L2 when the line is there.  xcd = the XCD the plan put this workgroup on (-1: not checked).
    int out_local, xcd, pad0;
    int bp_group, bp_slot0, bp_n, bp_blocks;   // LIN / FFN: the consumer's flags (group, first slot, count) and how many consecutive blocks make "all consumers"
    const float *w0, *w1;                 // S-format matrices
    const float *b0, *b1;                 // biases
    const float *g, *be;                  // LayerNorm gamma / beta
    const float *in0, *in1, *in2;         // block-layout activations: [NB][RT][256] (partials: [8][NB][RT][256])
    float* out;
    const float* bp_buf;                  // LIN / FFN, tagged hand-off: the consumer's OUTPUT rows (their tags are the ring's back-pressure)
};

// Geometry of one block, built on the host (sys_pack_blocks).  32-row tiles: both guidance branches of P prompts, T rows each
// (the latent count masks keys).  16-row tiles: ONE guidance branch of as many prompts as fit with only their count[b] valid
// latent rows (length-aware: padded latent rows never influence valid ones - they are masked as keys, every other op is
// per row, and ladiff.py:559-566 zeroes them at the end - so they are not computed at all).
struct BlockDesc {
    int nrows, nsb, pad0, pad1;
    int b2[16];                           // per sample-branch sx: text-cache row (-1: absent)
    // attention stage, per tile row: sx | first tile row of sx << 8 | valid latent keys << 16 (0xff: counts[] at run time); the
    // row's cross-attention / counts row (-1: padding)
    int row_pk[32], row_b2[32];
    int row_lat[32], row_t[32];           // latents row (prompt * T + t, -1: padding) and latent index of a tile row
    // reduce stages: part q of NRED handles slot k = wave + 4 i -> tile row | latent index << 8 | latent count << 16 (0xff: run
    // time), -1: no row; and the row's cross-attention table row.  The parts cover ALL rows of the tile: a row past nrows
    // (PART_PAD | row) is stored as zeros - under the tagged hand-off every row of a tile carries the step's parity, so that a
    // consumer checks whole tiles and needs no geometry.
    int part_pk[3][12], part_b2[3][12];
    // tail: (prompt, latent) pair k = wave + 4 i -> latents row (-1: none), latent index, tile row of the conditional branch.
    // A slot without a pair zeroes two padding rows instead: row pair_pad of the unconditional block and row pair_rc of the
    // conditional one (-1: nothing left to pad)
    int pair_lat[16], pair_t[16], pair_rc[16], pair_pad[16];
};
constexpr int PART_PAD = 0x40000000;
static_assert(NRED == 3, "BlockDesc::part_pk");
// How the reduce workgroups of a layer share a block's rows.  32-row blocks: NRED row parts each (<= 11 rows, 3 per wave).
// 16-row blocks: a part can take 8 rows (2 per wave), so RED2 needs only two workgroups and the freed one goes to STYL, the
// busiest stage of that plan: two GROUPS of two parts, group g visiting the blocks b = g (mod 2) - it sees every other block.
struct RedPlan { int red2_parts, styl_parts, styl_groups, out_groups; };
// how a layer's workgroups that hold no MLP slice are dealt (16-row blocks): variant 0 = one OUT workgroup, STYL as two groups on
// alternating blocks x two row parts; variant 1 = OUT as two groups on alternating blocks, STYL as one group x two row parts
constexpr RedPlan PLAN32{NRED, NRED, 1, 1}, PLAN16{2, 2, 2, 1}, PLAN16_OUT2{2, 2, 1, 2};
static_assert(PLAN32.styl_groups <= MAX_BP_BLOCKS && PLAN16.styl_groups <= MAX_BP_BLOCKS && PLAN16_OUT2.styl_groups <= MAX_BP_BLOCKS,
              "a ring's producer looks back at styl_groups consecutive blocks (Stage::bp_blocks): see PRING");
// The loop's measurement switches (include/ladiff_hip_debug.h, ladiff_debug_set_*): one process-wide object of atomics, defined in
// systolic_plan.hip.  Every value they accept selects a launch form that the tests hold to the same tolerances; the timing builds that
// produce garbage exist in the diagnostic twin only (-DLADIFF_STAMPS).  A launch reads them ONCE, as a LoopSwitches snapshot.
struct LoopSwitches {
    int waves16;                  // waves per SIMD of the 16-row plan's stage workgroups (ladiff_debug_set_stage_waves)
    int handoff;                  // hand-off of the 16-row plan's eight-wave stages: 1 = parity tags in the data, 0 = flags (ladiff_debug_set_handoff)
    int stage_plan;               // how a layer's spare workgroups are dealt (red_plan, ladiff_debug_set_stage_plan)
    int poll_pause, stage_delay;  // ladiff_debug_set_poll_pause / _stage_delay (mask | len << 8); stage_delay -1: by block count
    // ladiff_debug_set_pacing (eighths | mask << 8); -1: by block count - STYL sleeps half of its last observed wait before polling in launches above SMALL_LAUNCH_BLOCKS
    // (measured: -3 % at 128 / 256 prompts, round 4; -1.8 / -2.9 % at the round-6 kernels), nobody below (there pacing costs 0.4 %: profiles/r6/12_*)
    int pace;
    int look_ahead_from, small_upto;      // ladiff_debug_set_loop_thresholds (-1: LOOK_AHEAD_BLOCKS / SMALL_LAUNCH_BLOCKS)
    int xcd_local;                // ladiff_debug_set_xcd_local: 0 = no XCD placement, 1 = placed, 2 = placed and every workgroup reports a mismatch
};
struct LoopSwitchAtoms {
    std::atomic<int> waves16{2}, handoff{1}, stage_plan{0}, poll_pause{0}, stage_delay{-1}, pace{-1}, look_ahead_from{-1}, small_upto{-1}, xcd_local{1};
    LoopSwitches snapshot() const { return {waves16, handoff, stage_plan, poll_pause, stage_delay, pace, look_ahead_from, small_upto, xcd_local}; }
};
extern LoopSwitchAtoms g_loop;
inline RedPlan red_plan(int MR) { return MR != 1 ? PLAN32 : g_loop.stage_plan == 1 ? PLAN16_OUT2 : PLAN16; }
// sys_launch_policy's result: the key of the kernel instantiation (the rows of LOOP_KERNELS, systolic.hip) and the policy words of SysArgs
struct LoopKey { int mr, waves; bool tagged, look_ahead, fp32, multistep, edit, record = false; };   // mr: 1 | 2 = 16- | 32-row blocks (one form); waves per SIMD; look-ahead only with the tagged hand-off
inline bool operator==(const LoopKey& a, const LoopKey& b) {
    return a.mr == b.mr && a.waves == b.waves && a.tagged == b.tagged && a.look_ahead == b.look_ahead && a.fp32 == b.fp32 && a.multistep == b.multistep && a.edit == b.edit && a.record == b.record;
}
struct LoopLaunch { LoopKey key; int look_ahead, pace, delay_mask, delay_len, pause_mask, pause_len, force_mismatch; };
// record: the call records its trajectory (the RC rows of LOOP_KERNELS): those have no look-ahead form, so a tagged recording launch runs
// without look-ahead whatever its block count
LoopLaunch sys_launch_policy(int MR, int NB, bool fp32, bool multistep, bool edit, const LoopSwitches& sw, bool record = false);

struct SysLayout {
    size_t blk, ring;             // floats of one [NB][RT][256] buffer / of one [PRING][RT][256] partial plane
    size_t off_stages, off_blocks, off_flags, off_status, off_xin0, off_xs, off_xo, off_att, off_x1, off_x2, off_pc, off_pe, total;
    int nwg, NB, split;
};

// ---- the planner (systolic_plan.hip): integer and pointer arithmetic on the host, no HIP call
SysLayout sys_layout(int MR, int NB);
int plan_nwg(int MR);
int prompts_per_block32(int T);
int nb32(int B, int T);
int nb16_max(int B, int T);
size_t sys_ws_floats(int B, int T);
void sys_pack_blocks(int B, int T, int want_mr, const int32_t* h_counts, bool masked, bool cfg, std::vector<unsigned char>& out, int* mr, int* nb);
void sys_place_stages(std::vector<Stage>& st, bool round_robin);
int sys_build_stages(const DenoiserW& W, const DenoiserW& WS, float* ws, int MR, int NB, bool round_robin, std::vector<unsigned char>& host);
size_t sys_blocks_offset_floats(int MR, int NB);
size_t sys_status_offset_floats(int B, int T);
void choose_plan(int B, int T, const int32_t* h_counts, bool masked, int loop_mode, bool f16x3, std::vector<unsigned char>& plan,
                 int* plan_mr, int* plan_nb, bool cfg = true);

}  // namespace ladiff
