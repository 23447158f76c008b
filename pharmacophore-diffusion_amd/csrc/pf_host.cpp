// pf_host.cpp -- C ABI of libpfdyn.so (include/pfdyn.h): handle, weight commit (the packer itself: pf_pack.cpp), workspace,
// launch sequencing.  No compute happens on the host; without a HIP device every compute entry
// point fails (there is no CPU fallback).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <string>
#include <unordered_map>
#include <climits>
#include <vector>

#include "../../include/pfdyn.h"
#include "pf_device.h"
#include "pf_bind.h"
#include "pf_pack.h"
#include "pf_train.h"
#include "pf_score.h"
#include "pf_optim.h"
#include "pf_field.h"
#include "pf_restr.h"
#include "pf_types.h"
#include "pf_pairs.h"
#include "pf_sset.h"
#include "pf_align.h"
#include "pf_mem.h"

using namespace pfpack;

#define L0_PTAB_SLOTS 2048        // timesteps whose layer-0 type tables stay resident (pf_prepare_timesteps)

extern "C" {
void pfk_edge_msg(const EdgeParams* p, int layer0, hipStream_t s);
void pfk_edge_msg_coop(const EdgeParams* p, int layer0, hipStream_t s);
void pfk_edge_msg_coop2(const EdgeParams* p, int layer0, hipStream_t s);
void pfk_node_update_coop(const NodeParams* p, int layer0, hipStream_t s);
void pfk_node_head_coop(const NodeParams* p, const HeadParams* hp, int layer0, hipStream_t s);
void pfk_noise_head_coop(const HeadParams* p, hipStream_t s);
void pfk_node_update(const NodeParams* p, int layer0, hipStream_t s);
void pfk_noise_head(const HeadParams* p, hipStream_t s);
void pfk_rg_edge(const EdgeParams* p, const EncodeParams* enc, int layer0, int rg, int split, int rgp, hipStream_t s);
void pfk_l0_hoist(const L0HoistParams* p, int what, hipStream_t s);
void pfk_rg_node(const NodeParams* p, const HeadParams* hp, const EncodeParams* enc, int layer0, int rg, int split, hipStream_t s);
void pfk_rg_unit(const UnitParams* p, hipStream_t s);
void pfk_rg_node_hs_build(const NodeParams* p, const HeadParams* hp, const StepParams* sp, const BuildParams* bp, int* xstat, int poll_sleep,
                          int avoid, int poll_max, const CenHoistParams* cp, const EdgeParams* es, const EncodeParams* ees, int spec_groups,
                          hipStream_t s);
void pfk_n16_edge(const EdgeParams* p, const EncodeParams* enc, int layer0, hipStream_t s);
void pfk_pa_spec(const EdgeParams* es, const EncodeParams* ees, int groups, int after, int k, int frac, int* word, hipStream_t s);
void pfk_pa_check(const int* dyn_cnt, const int* cnt_snap, const int* reg, const int* pa_same, const int* gstamp, int serial, int B,
                  unsigned long long* out, hipStream_t s);
void pfk_n16_unit(const UnitParams* p, hipStream_t s);
void pfk_n16_fused(const EdgeParams* p, const FusedParams* f, const EncodeParams* enc, hipStream_t s);
void pfk_n16_tail(const TailParams* t, const StepParams* sp, const BuildParams* bp, hipStream_t s);
void pfk_rg_tail(const NodeParams* p, const HeadParams* hp, const StepParams* sp, const BuildParams* bp, hipStream_t s);
void pfk_encode(const EncodeParams* p, hipStream_t s);
void pfk_encode_build(const EncodeParams* e, const BuildParams* b, hipStream_t s);
void pfk_encode_build_pre(const EncodeParams* e, const BuildParams* b, const PreParams* pp, hipStream_t s);
void pfk_build_edges(const BuildParams* p, hipStream_t s);
void pfk_load_coords(const float* src, float4* xn, int n, const int* gid, const float* shift, float sign, hipStream_t s);
void pfk_load_noise0(const float* nz, float4* xn, float* hf, int n, int nf, hipStream_t s);
void pfk_copy(const float* src, float* dst, size_t n, hipStream_t s);
void pfk_zero_multi(const ZeroList* z, hipStream_t s);
void pfk_copy2(const float* a, float* da, size_t na, const float* b, float* db, size_t nb, hipStream_t s);
void pfk_verify_copies(const float* x0, const float* h0, const int* gid, const int* prot_ptr, const int* rep_base, int Np, int rec_nf,
                       int* flag, hipStream_t s);
void pfk_scale_copy(const float* src, float* dst, size_t n, float sc, hipStream_t s);
void pfk_segment_mean(const float4* xn, const int* ptr, int base, int B, float* out, hipStream_t s);
void pfk_step_build_fast(const StepParams* sp, const BuildParams* bp, hipStream_t s);
void pfk_step_move(const StepParams* sp, const StepMoveArgs* a, const BuildParams* bp /* NULL: the move alone */, hipStream_t s);
void pfk_guide_grad(const StepParams* p, const GuideParams* q, hipStream_t s);
void pfk_guide_field(const StepParams* p, const FieldParams* q, hipStream_t s);
void pfk_guide_field_types(const StepParams* p, const FieldParams* q, const FieldTypeParams* ft, hipStream_t s);
void pfk_guide_types(const StepParams* p, const TypeParams* q, hipStream_t s);
void pfk_guide_pairs(const StepParams* p, const PairParams* q, hipStream_t s);
void pfk_sset_analyze(const SsetParams* q, int work_items, hipStream_t s);
void pfk_pharm_align(const AlignParams* q, hipStream_t s);
void pfk_pin_restore(const int* flags, const float* pin_x, const float* pin_h, int n, int nf, float* out_x, float* out_h, hipStream_t s);
void pfk_export_coords(const float4* xn, int base, int n, const int* gid, const float* add, const float* sub,
                       float* out, hipStream_t s);
void pfk_bwd_head(const BwdHeadParams* p, int nblocks, hipStream_t s);
void pfk_bwd_node(const BwdNodeParams* p, int nblocks, hipStream_t s);
void pfk_bwd_edge_level(const BwdEdgeLevelParams* p, int nblocks, hipStream_t s);
void pfk_fix_apply(long long* A, float* G, size_t n, const float* fix, hipStream_t s);
void pfk_fix_apply_rows(const NodeTile* tiles, int ntiles, const int* dyn_cnt, const int* row_ids, long long* A_h, float* G_h,
                        long long* A_v, float* G_v, const float* fix, hipStream_t s);
void pfk_fix_scale(const float* g_h, int n_h, const float* g_x, int n_x, float* fix, hipStream_t s);
void pfk_bwd_encode(const BwdEncodeParams* p, int nblocks, hipStream_t s);
void pfk_enc_group(const float* G_h, const int* prot_ptr, const int* ptype, int B, int rec_nf, float* Gg, hipStream_t s);
void pfk_fix_enc_group(long long* A_h, float* G_h, const float* fix, const int* prot_ptr, const int* ptype, int B, int rec_nf, float* Gg,
                       int Np, int Nf, const int* onehot_flag, hipStream_t s);
void pfk_train_reduce(const ReduceParams* p, hipStream_t s);
void pfk_gather_weights(const float* flat, const int* map, size_t n, float* packed, hipStream_t s);
void pfk_n16_split_words(const float* flat, const int4* tab, size_t n, float* packed, hipStream_t s);
void pfk_pack_gvp(const float* W, const GvpT* g, int n_gvps, float* out_b, float* out_f, const ScaleArgs* sa, hipStream_t s);
void pfk_loss_prepare(const LossParams* p, hipStream_t s);
void pfk_loss_eval(const LossParams* p, int ep_coord, int ep_feat, hipStream_t s);
void pfk_score_prepare(const ScoreParams* p, hipStream_t s);
void pfk_score_eval(const ScoreParams* p, int ep_coord, int ep_feat, hipStream_t s);
void pfk_scale_loss(float* gx, int nx, const float* a, const float* a2, float* gh, int nh, const float* b, const float* b2, hipStream_t s);
void pfk_compact_node_rows(const NodeTile* tiles, int ntiles, const int* dyn_cnt, const int* row_ids, int N, int* list, int cap, int* ucnt,
                           hipStream_t s);
void pfk_compact_rows(const EdgeTile* tiles, const int* et_tile0, int n_et, const int* dyn_cnt, int* rlist, int* ccnt, hipStream_t s);
void pfk_adam(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2, float eps, float wd,
              float bc1, float bc2_sqrt, float* mirror, hipStream_t s);
void pfk_drop_masks(const TrainCommon* c, uint32_t stream, int n_elems, float* out, hipStream_t s);
void pfk_pp_radius(const float4* xn, const int* prot_ptr, int B, float r2, int maxn, int* deg, const int* row_off,
                   int* src, int* dst, int pass, hipStream_t s);
// width-generic family (pf_wide.hip)
void pfk_wide_encode(const WideEncParams* p, hipStream_t s);
void pfk_wide_pack(const float* flat, const WidePackJob* jobs, int n_jobs, float* out, hipStream_t s);
void pfk_wide_edge(const WideEdgeParams* p, int train, hipStream_t s);
void pfk_wide_node(const WideNodeParams* p, int train, hipStream_t s);
// its gradient kernels (pf_wide_train.hip)
void pfk_wt_chain(const WtChainParams* p, int edge, int wgrad, hipStream_t s);
void pfk_wt_norm(const WtNormParams* p, int wgrad, hipStream_t s);
void pfk_wt_head_out(const WtHeadOutParams* p, int wgrad, hipStream_t s);
void pfk_wt_encode(const WtEncParams* p, int wgrad, hipStream_t s);
void pfk_wt_reduce(const float* gpart, int gstride, float* grad, int nparams, hipStream_t s);
// both training families (pf_wide_train.hip; the kernel reads the edge-slot layout they share): dL/d(center coordinates) from the
// per-edge dL/d(x_src - x_dst) rows their level-0 launches leave
void pfk_wt_center_sum(const WtCenterSumParams* p, hipStream_t s);
}

namespace {

static std::string g_create_error;

// torch.linspace(start, end, steps) in fp32 (symmetric evaluation like ATen)
static void linspace_f32(float start, float end, int steps, float* out) {
    const float step = (end - start) / (float)(steps - 1);
    const int half = steps / 2;
    for (int i = 0; i < steps; ++i) out[i] = i < half ? start + step * (float)i : end - step * (float)(steps - i - 1);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// Launch policy of the inference path: which kernel form a launch takes.  One place, one table.  The rows are implemented by the pieces of
// run_dynamics: the edge rows by edge_launch (n16 form: edge_n16_form; row 1: fused_take_node), the node and "nodes + head" rows by node_launch
// (bit 3's launch: tail_launch; the merged last launch of a denoising step: merged_step_launch), a head of its own by head_launch.
//
// The chip: 256 compute units (CUs) = 1,024 SIMDs.  A launch is in the LATENCY regime while it has about as many items
// as the chip has places to put them (its duration is one item's chain of dependent GVPs), in the THROUGHPUT regime beyond.
// Sizes below are EDGE SLOTS (or node rows) of the launch's work list = 32 x its tiles: capacities, known on the host
// (the dynamic edge counts are not; at 256-atom pockets with kNN pf edges about a third of the slots hold an edge).
//
//   launch                        | size (slots / rows)        | form
//   ------------------------------+----------------------------+---------------------------------------------------------
//   conv layer 0's node update    | batch <= n16_fuse_rows_max | none: computed by the last layer's edge items for their own source rows
//     (n_convs = 2, kNN pf edges) |   (20,000: <= 32 graphs)   |   (pf_n16.hip: k_n16_fused; one launch less per step)
//   edge messages, any conv layer | batch <= n16_rows_max      | n16: 16-row items on the four waves of a workgroup
//                                 |   (24,000 ~ 2 busy items   |   (pf_n16.hip; conv layer 0 needs the static hoist's type
//                                 |   per CU)                  |   tables, else the row-group form)
//   edge messages                 | < rg2_rows_min (12,000 ~   | row-group, 4 rows per wave (pf_rg.hip); four-wave workgroups
//                                 |   3 four-row items / SIMD) |   up to RG_QUAD_MAX item slots (fixed SIMD placement)
//                                 | >= rg2_rows_min            | row-group, 8 rows per wave
//     conv layer 0 under the      | >= rg2p_rows_min (11,000)  |   hoisted (two-block) items 8 rows, full-chain items 4
//     static hoist (compact list) | >= rg2_rows_min_hoist      |   all items 8 rows
//                                 |   (30,000)                 |
//   node update                   | < rg2_rows_min_node        | row-group, 4 rows per wave; on TWO waves per item while the
//                                 |                            |   launch has <= rg_split_max_node (256) items: fewer items than CUs
//                                 | >= rg2_rows_min_node       | row-group, 8 rows per wave
//   last layer's nodes + head     | <= rg_split_max_head (512) | row-group, 4 rows on two waves (a 6-7 block chain: the longest of a step)
//   everything, row-group off     | rows > rg_rows_max         | 32-row tile kernels (pf_kernels.hip): four waves per tile up to
//   (training forward of dense    |                            |   coop_edge_max / coop_node_max tiles, two workgroups per CU up to
//   layers; PFDYN_RG_ROWS_MAX=0)  |                            |   coop2_*_max, one wave per tile beyond
//
// Every threshold can be overridden from the environment (tests force every form onto the goldens; sweeps: tools/):
//   PFDYN_N16 (bit 0: conv layers >= 1, bit 1: conv layer 0, bit 2: conv layer 0's node update fused into the last layer's edge launch when
//   n_convs = 2, bit 3: the tail launch of a denoising step -- last node update + noise head + sampler update + edge build, one workgroup per
//   graph: off unless asked for; default 7), PFDYN_TAIL_GRAPHS_MAX, PFDYN_TAIL_FORM (rg | n16), PFDYN_N16_ROWS_MAX (sets both n16 thresholds),
//   PFDYN_N16_FUSE_ROWS_MAX, PFDYN_RG_ROWS_MAX, PFDYN_RG2_ROWS_MIN (sets all four 8-row thresholds) / _NODE / _HOIST, PFDYN_RG2P_ROWS_MIN,
//   PFDYN_L0_RGA / PFDYN_L0_RGP (rows-per-wave factor of the full-chain / hoisted items of a compact layer-0 launch), PFDYN_RG_SPLIT_MAX (all
//   three) / _NODE / _HEAD, PFDYN_COOP_EDGE_MAX, PFDYN_COOP2_EDGE_MAX, PFDYN_COOP_NODE_MAX.  Forcing a row-group form switches the n16 form
//   off unless PFDYN_N16 is given.  Feature switches (not thresholds) are read in pf_handle::init_tuning.
// ------------------------------------------------------------------------------------------------------------------
struct LaunchPolicy {
    static constexpr int kCUs = 256, kSIMDs = 4 * kCUs;
    // bit 3: the tail launch (node update of the last layer + noise head + sampler update + edge build in one launch, one workgroup per
    // graph).  OFF by default: measured on config 2 it LOSES to the separate launches in both forms -- 30.7 us (row-group form: two
    // two-wave items per compute unit stream 192 KB of weights per block through one CU's memory path) and 28.0 us (n16 form: 2.0 us
    // per block on a 16-row tile that holds six centers) against 14.7 + 10.3 us (profiles/r04/tail_forms.txt)
    int n16_mask = 7;
    int tail_graphs_max = 256;              // ... up to this many graphs (one four-wave workgroup per graph; it does not share a CU)
    // k_n16_fused: ff / store items on XCDs 0..3, pf items on XCDs 4..7 -- an XCD's L2 fetches half of the launch's weights: 19.3 -> 18.5 us
    // at config 2 (PFDYN_XCD_SPLIT=0: off).  The same idea on the conv-layer-0 launch (pa / pf items on five XCDs, ff / fp items on three)
    // LOST 1.6 us: that launch is throughput-bound with two items per compute unit, and the split unbalances it (profiles/r04)
    int xcd_split = 1;
    int edge_rec = 1;                          // PFDYN_EDGE_REC: edge records for the fused launch (BuildParams::rec)
    int node_static = 1;                    // ... with its tiles computed, not loaded (k_rg_node_hs; PFDYN_NODE_STATIC=0: the tile-list kernel)
    int node_xcds = 2;                      // the fused node + head launch of a small batch runs on this many XCDs (PFDYN_NODE_XCDS; 0: all eight)
    int fused_uni = 1;                      // the fused launch's arithmetic tiling when every graph's regions have one capacity (PFDYN_FUSED_UNI)
    int xchg_sleep = 1, hsb_avoid = 0;      // its poll interval in units of ~0.2 us (PFDYN_XCHG_SLEEP); update + build workgroups kept off the first n XCDs (PFDYN_HSB_AVOID)
    int hs_build = 1;                       // the merged last launch of a step (k_rg_node_hs_build: node + head items and the update + build of every
                                            // graph as workgroups of one grid; PFDYN_HS_BUILD=0: two launches)
    int tail_form = 4;                      // 4: the row-group form (k_rg_tail: two two-wave items of four centers), 16: the n16 form (k_n16_tail)
    long n16_fuse_rows_max = 20000;         // the fused launch (bit 2): +2-3 % up to 32 graphs of 256 atoms, -4 % at 40 (its items carry five blocks: throughput-bound earlier)
    long n16_rows_max = 24000;              // measured at 256-atom pockets (575 slots per graph): +5 % at 16 graphs, +10 % at 32, -3..-5 % at 64, -15 % at 256
    int rg_rows_max = 1 << 30;
    int rg2_rows_min = 12000;               // ~3 four-row items per SIMD (3 x 4 x kSIMDs = 12,288)
    int rg2_rows_min_node = 12000;
    int rg2p_rows_min = 11000;              // mixed 4 / 8 rows: +5 % at 24 graphs, +2 % at 32, +7 % at 40, +11 % at 48 over all-4-rows (round 2 sweep)
    int rg2_rows_min_hoist = 30000;         // all-8-rows: +10 % at 56-64 graphs
    int l0_rga = 0, l0_rgp = 0;             // 0: by the thresholds above
    int rg_split_max = 128;                 // edge launches: two waves per 4-row item up to this many items (kCUs / 2)
    int rg_split_max_node = 256;            // = kCUs
    int rg_split_max_head = 512;            // = 2 kCUs: +2-3 % at 144-384 items
    int coop_edge_max = 256, coop_node_max = 1024;       // tile kernels: one tile per CU / per SIMD
    int coop2_edge_max = 12000, coop2_dense_max = 1024;
    // 0: tile kernels; 1 / 2: row-group kernels with 4 / 8 rows per wave
    int rg_mode(int ntiles) const {
        const long rows = (long)ntiles * 32;
        if (rows > rg_rows_max) return 0;
        return rows >= rg2_rows_min ? 2 : 1;
    }
    void from_env() {
        auto geti = [](const char* v, int& x) { if (const char* e = getenv(v)) x = atoi(e); };
        geti("PFDYN_COOP_EDGE_MAX", coop_edge_max); geti("PFDYN_COOP_NODE_MAX", coop_node_max);
        if (const char* e = getenv("PFDYN_COOP2_EDGE_MAX")) coop2_edge_max = coop2_dense_max = atoi(e);
        if (const char* e = getenv("PFDYN_RG_SPLIT_MAX")) rg_split_max = rg_split_max_node = rg_split_max_head = atoi(e);
        geti("PFDYN_RG_SPLIT_MAX_NODE", rg_split_max_node); geti("PFDYN_RG_SPLIT_MAX_HEAD", rg_split_max_head);
        geti("PFDYN_RG_ROWS_MAX", rg_rows_max);
        if (const char* e = getenv("PFDYN_RG2_ROWS_MIN")) rg2_rows_min = rg2_rows_min_hoist = rg2p_rows_min = rg2_rows_min_node = atoi(e);
        geti("PFDYN_RG2P_ROWS_MIN", rg2p_rows_min); geti("PFDYN_RG2_ROWS_MIN_NODE", rg2_rows_min_node); geti("PFDYN_RG2_ROWS_MIN_HOIST", rg2_rows_min_hoist);
        geti("PFDYN_L0_RGP", l0_rgp); geti("PFDYN_L0_RGA", l0_rga);
        for (const char* v : {"PFDYN_RG2_ROWS_MIN", "PFDYN_RG2P_ROWS_MIN", "PFDYN_RG2_ROWS_MIN_HOIST", "PFDYN_RG_SPLIT_MAX", "PFDYN_L0_RGA",
                              "PFDYN_L0_RGP", "PFDYN_RG_ROWS_MAX"})
            if (getenv(v)) n16_mask = 0;
        geti("PFDYN_N16", n16_mask);
        geti("PFDYN_TAIL_GRAPHS_MAX", tail_graphs_max);
        geti("PFDYN_XCD_SPLIT", xcd_split);
        geti("PFDYN_EDGE_REC", edge_rec);
        geti("PFDYN_NODE_XCDS", node_xcds); geti("PFDYN_NODE_STATIC", node_static); geti("PFDYN_HS_BUILD", hs_build); geti("PFDYN_FUSED_UNI", fused_uni); geti("PFDYN_XCHG_SLEEP", xchg_sleep); geti("PFDYN_HSB_AVOID", hsb_avoid);
        if (const char* e = getenv("PFDYN_TAIL_FORM")) tail_form = (e[0] == 'n' || atoi(e) == 16) ? 16 : 4;
        if (const char* e = getenv("PFDYN_N16_ROWS_MAX")) n16_rows_max = n16_fuse_rows_max = atol(e);
        if (const char* e = getenv("PFDYN_N16_FUSE_ROWS_MAX")) n16_fuse_rows_max = atol(e);
    }
};

// which sampling run is in progress on a handle (run_guard: what each entry point accepts)
enum RunKind { RUN_NONE = 0, RUN_PLAIN, RUN_PINNED, RUN_GUIDED };

// What owns the handle's memory, events and streams (pf_mem.h).  StagedBlock: a block of host arrays that a guided begin uploads in
// one copy (the restraints, the pocket field, type guidance) -- its device buffer is kept and grown like d_pin
using pfmem::DevArr; using pfmem::DevBuf; using pfmem::Event; using pfmem::PinnedArr; using pfmem::PinnedBuf; using pfmem::StagedBlock;
using pfmem::Stream; using pfmem::Wait;

struct pf_handle {
    // ---- optional per-kernel timing with HIP events on the caller's stream (pf_profile_*)
    // classes 0..8: pf_profile_read (inference path); 9..12: pf_profile_read_train (gradient kernels)
    enum { K_ENCODE = 0, K_BUILD, K_EDGE, K_NODE, K_HEAD, K_STEP, K_EDGE_COOP, K_NODE_COOP, K_EDGE_LAST,
           K_BWD_HEAD, K_BWD_NODE, K_BWD_EDGE_LEVEL, K_BWD_REST, K_NUM };
    // ---- streams, events and the two alternating pairs.  Members are destroyed in reverse order of declaration, and these are
    // declared first: every buffer further down goes before them, then the pairs (buffer, then events), the events, the streams
    Stream s_copy;                          // the table section's upload (below)
    Stream s_side;                          // side stream of the backward pass (work lists, early gradient sums, encoders): NOT the copy
                                            // stream -- the next bind's upload must not queue behind the end of this backward
    std::vector<std::pair<Event, Event>> prof_ev[K_NUM];
    Event cmp_ev[3];                        // the backward pass's side stream against the caller's (bwd_side_lists, bwd_early_reduce)
    Event l0flag_ev;                        // the read-back into l0flag_host
    // pf_set_pocket_batch stages every host-built table in pinned memory, in the layout of the workspace's table section,
    // and uploads it with ONE asynchronous copy (two staging buffers alternate; a buffer is reused only after the copy that
    // read it has completed: ev)
    struct StageSlot { Event ev; PinnedBuf buf; } stage[2];
    int stage_next = 0;
    // The table section lives in two device buffers of its own that alternate between binds, and its upload runs on a
    // copy stream: a training loop binds a new batch every step, and on the caller's stream the ~8 MB copy would sit
    // between two steps (0.14 ms of a 2 ms step) instead of under the previous step's kernels.  guard: everything
    // that read the buffer has finished (recorded on the caller's stream at the start of the bind after the one that
    // used it; forgotten when the buffer is replaced); up: the upload into it is complete (the caller's stream waits for it).
    struct TabSlot { Event guard, up; DevBuf buf; } tab[2];
    int tab_next = 0;

    LaunchPolicy pol;
    pf_config cfg{};
    // width-generic family (pf_wide.hip): every inference call of a handle whose widths are not (128, 16) runs on it, and so does
    // a (128, 16) handle created under PFDYN_WIDE=1.  spec: the widths of the specialised kernels -- their weights are packed and
    // training is available; wide: inference goes to run_dynamics_wide
    bool spec = true, wide = false;
    DevArr<WideGvp> d_wgvp;                 // device table of the width-generic GVPs (same indexing as d_gvp)
    std::string err;
    std::map<std::string, RawTensor> raw;
    bool committed = false;

    // ---- packed weights (one device allocation)
    DevArr<float> d_w;
    PackLayout pk;                          // where everything sits in d_w (pf_pack.h): offsets and strides in floats
    DevArr<GvpW> d_gvp;                     // table of all GvpW
    std::vector<GvpW> h_gvp;
    // indices into the GvpW table
    int msg_base(int layer, int et) const { return ((layer * 4 + et) * cfg.n_message_gvps); }
    int upd_base(int layer, int nt) const { return n_msg_tot + (layer * 2 + nt) * cfg.n_update_gvps; }
    int head_base() const { return n_msg_tot + n_upd_tot; }
    int n_msg_tot = 0, n_upd_tot = 0;
    bool use_pre = true;

    // ---- batch / workspace
    bool have_batch = false;
    int B = 0, Np = 0, Nf = 0, N = 0;
    int64_t Epp = 0, Ecap = 0;
    std::vector<int> h_prot_ptr, h_pharm_ptr;
    std::vector<int> h_reg;                 // [4][B] first slot of the ff, pf, fp and pa regions
    std::vector<int> h_cap;                 // [4][B] ... and their capacities
    int n_edge_tiles = 0, n_node_tiles = 0, n_head_tiles = 0;
    int zero_row = 0;
    int n_edge_tiles_last = 0, n_node_tiles_last = 0;
    // receptive-field pruning of the second-to-last conv layer: only the protein atoms that are the source of a
    // pf edge (the only protein rows the last layer reads) are updated, and only the edges into them are computed
    bool prune = true;
    int n_edge_tiles_act = 0, n_node_tiles_act = 0;
    EdgeTile* d_edge_tiles_act = nullptr;
    NodeTile* d_node_tiles_act = nullptr;
    int *d_act_ids = nullptr, *d_reg_act = nullptr;   // last conv layer: only what feeds the pharm nodes
    DevBuf d_ws;                            // one allocation, carved below; kept across pocket batches while it is large enough
    // one-hot check of the protein features (static hoist): 0 unknown (device flag pending), 1 one-hot, 2 not
    int l0_state = 0;
    PinnedArr<int> l0flag_host;             // written by an async copy of d_l0flag
    int *d_prot_ptr = nullptr, *d_pharm_ptr = nullptr, *d_gid = nullptr, *d_reg = nullptr, *d_dyn_cnt = nullptr,
        *d_esrc = nullptr, *d_edst = nullptr, *d_in_start = nullptr, *d_in_cnt = nullptr, *d_pp_cnt = nullptr;
    EdgeTile* d_edge_tiles = nullptr;
    NodeTile* d_node_tiles = nullptr;
    NodeTile* d_head_tiles = nullptr;
    float4* d_xn = nullptr;
    float *d_prot_x0 = nullptr, *d_prot_h0 = nullptr, *d_pharm_h = nullptr, *d_t = nullptr, *d_h[2] = {nullptr, nullptr},
          *d_v[2] = {nullptr, nullptr}, *d_msg_s = nullptr, *d_msg_v = nullptr, *d_eps_h = nullptr, *d_eps_x = nullptr,
          *d_com_init = nullptr, *d_com_tmp = nullptr, *d_gnorm = nullptr, *d_pre = nullptr;
    int* d_pfq_cnt = nullptr;      // [B] reference-booked pf edge counts (message_norm 0 with kNN pf edges), else NULL
    // pocket sharing: pf_set_pocket_groups names, per graph, the representative graph of its pocket; the
    // next bind verifies the claim and, when it pays, prepares the tables of the sharing mode
    std::vector<int> pending_rep;           // consumed by the next pf_set_pocket_batch*
    bool share_ok = false;                  // tables of the sharing mode exist for this batch
    int share_check = 1;                    // the claim's rows: 1 verified (host rows, or nothing claimed), 0 compared on the device and not
                                            // read back yet (l0flag_host[1], behind l0flag_ev), 2 found false
    int* d_reg_share = nullptr;             // [4][B]: d_reg with the kind-3 entries of representatives at their static pp edges
    int* d_pa_static = nullptr;             // [B]: static pp edge count of a representative, 0 for a copy
    int* d_rep_base = nullptr;              // [B]: node id of the first atom of each graph's representative
    int* d_need = nullptr;                  // [Np]: stamp of the last build in which some copy had the atom active
    int need_stamp = 0, edges_stamp = 0;    // stamp of the next build / of the build the current edges came from
    long share_rows = 0;                    // edge slots of a shared layer-0 launch (capacities of ff, pf, fp + the static ranges)
    std::vector<int> h_share_start, h_share_cnt;   // host copies of d_reg_share's kind-3 entries / d_pa_static (grid sizing)
    bool share_disable = false;             // PFDYN_NO_POCKET_SHARE=1
    bool train_rg_node = true;              // PFDYN_TRAIN_TILE_NODE=1: the training forward keeps the 32-row tile node kernel
    bool train_rg_edge = true;              // PFDYN_TRAIN_TILE_EDGE=1: ... and the 32-slot tile edge kernel
    bool train_rg_head = true;              // PFDYN_TRAIN_TILE_HEAD=1: the training forward's noise head on the tile kernel (the backward recomputes it)
    float *t_hsv_z = nullptr, *t_hsv_g = nullptr, *t_hsv_v = nullptr;   // head levels saved by the training forward [n_noise_gvps][Nf][128 / 16 / 48]
    bool t_head_saved = false;              // ... by the last pf_train_forward
    unsigned int* d_xchg = nullptr;         // exchange words of the merged launch [Nf centers][PF_XCHG_STRIDE]: part of the workspace (carved per
                                            // bind), set to PF_XCHG_EMPTY by every pf_sample_begin on the caller's stream, re-armed word by word by the consumers
    DevArr<int> d_xstat;                    // [1] time-outs of the exchange since the handle was created (cumulative, never cleared: no race with a run in flight)
    PinnedArr<int> xstat_host;              // an async copy of d_xstat follows every sampling run (pf_sample_end)
    int xstat_ack = 0;                      // the count already reported (pf_sample_status / pf_sample_begin / pf_debug_xchg_timeouts)
    int xchg_fault = 0, xchg_poll_max = 0;  // diagnostics (pf_debug_xchg_fault)
    // center hoist (CenHoistParams; pf_cenhoist.h; its streams and L0C block: pk.n16_l0h, pk.l0c_off): the per-batch
    // tables and exchange copy, two alternating snapshots of the centers' features, the announced timestep plan (pf_prepare_timesteps)
    // that tells a denoising step the NEXT call's t, and what the tables currently hold
    bool cen_hoist = true;                  // PFDYN_NO_CENTER_HOIST=1: off
    float *d_cen_h = nullptr, *d_cen_p = nullptr, *d_snap[2] = {nullptr, nullptr};
    unsigned int* d_xchg2 = nullptr;
    int snap_cur = -1;                      // which snapshot holds the features as they are now (-1: none)
    std::vector<float> t_plan; size_t plan_pos = 0;
    bool cen_valid = false; float cen_t = 0.f; uint64_t cen_wver = 0;
    bool last_cen = false;                  // the last dynamics call started its ff / fp items from the tables (pf_debug_kernel_family(n_convs + 1))
    // speculative "pa" messages (BuildParams::pa_same, k_n16_pa_spec): a side stream, the events that order it against the caller's
    // stream, a per-handle step counter (never reset: stamps of an earlier trajectory must not look recent), the conv-layer-0 launch's
    // parameters of the current call, and what the rows computed ahead are for
    bool pa_spec = true;                    // PFDYN_NO_PA_SPEC=1: off
    bool spec_valid = false; float spec_t = 0.f; uint64_t spec_wver = 0;
    int step_id = 2;
    int *d_pa_stamp = nullptr, *d_pa_same = nullptr;
    bool e0_saved = false; EdgeParams e0{}; EncodeParams ep0{}; int e0_groups = 0;
    int last_spec = 0;                      // the last dynamics call skipped "pa" regions computed ahead (pf_debug_kernel_family(n_convs + 2): 1)
    int last_forms = 0;                     // item maps of the last dynamics call's n16 launches (pf_debug_kernel_family(n_convs + 3)): bit 0 conv layer 0 ran
                                            // k_n16_edge_u, bit 1 the fused launch ran k_n16_fused_u, bit 2 the fused launch's items started from edge records
                                            // when the next one begins: a time-out there is reported, late but never silently
    int* d_pa_cnt = nullptr;                // [B] the kind-3 counts conv layer 0 consumed (EdgeParams::cnt_snap): the speculative items' map
    // test knobs.  PFDYN_PA_SPEC_SPLIT=k: the speculative items leave the merged launch; items w < k run in a launch of their
    // own just before it (the counts before the build), items w >= k just after it (the counts after the build); k > 0 fixed, "mid": half of
    // the non-empty groups, "step": a fraction of them the host picks per step.  PFDYN_PA_CHECK=1: every speculative item stamps its group with the serial
    // of the launch it belongs to, and a check in front of the next call's conv layer 0 counts the kept groups whose stamp is not that serial
    int pa_spec_split = 0;                  // 0 off, > 0 fixed k, -1 mid, -2 per step
    bool pa_check = false;
    int pa_serial = 0, spec_serial = 0;
    int* d_pa_gstamp = nullptr;             // [Ecap / 16 + 1] in the workspace (PFDYN_PA_CHECK only)
    DevArr<unsigned long long> d_pa_chk;    // [3] violations, kept groups checked, kept groups behind a changed prefix (per handle, cumulative)
    bool no_fixed_shapes = false;           // PFDYN_NO_FIXED_SHAPES: k_bwd_edge_level reads every level's GVP shape from the table (the A/B of its FX forms)
    ScaleArgs pend_scale{}; bool has_pend_scale = false;    // loss_backward -> pf_train_backward: the unit gradients' scaling, not yet launched
    bool vjp_full_kernels = false;          // PFDYN_VJP_FULL_KERNELS: the inputs-only backward launches the full pass's kernel forms (the A/B of the
                                            // kernel-level skip; the host-level skip -- no clear, no reduce -- stays)
    bool no_fix_fuse = false;               // PFDYN_NO_FIX_FUSE: k_fix_apply and k_enc_group as two launches (the A/B of k_fix_enc_group)
    bool train_bf16 = false;                // pf_train_set_precision: the bf16 leg (dense Linears of the message chains' forward and of every
                                            // gradient kernel on bf16 matrix instructions; PFDYN_TRAIN_BF16=1 sets it at creation)
    bool train_node_save = true;            // PFDYN_TRAIN_NODE_RECOMPUTE=1: k_bwd_node recomputes the update chains instead of reading saved levels
    std::vector<float*> t_nsv_z, t_nsv_g, t_nsv_v;  // per conv layer: update-chain levels saved by the training forward [n_update_gvps][2 N][128 / 16 / 48]
    std::vector<char> t_node_saved;         // ... by the last pf_train_forward
    std::vector<int> t_grp;                 // per conv layer: slots per message partial-row group of the last training forward
    RunKind run = RUN_NONE;                 // set by the three pf_sample_begin* calls, reset by a bind
    // pinned centers (pf_sample_begin_pinned): the run in progress replaces the flagged centers every step; the handle's own copy of
    // the caller's arrays (one allocation, kept and reused: flags [Nf], positions [Nf][3], feature rows [Nf][pharm_nf])
    DevBuf d_pin;
    int* d_pin_flags = nullptr; float *d_pin_x = nullptr, *d_pin_h = nullptr;
    float pin_feat_norm = 1.f;
    // seeded begin (pf_sample_seed_next): the handle's own copy of the caller's seed (one allocation, kept and grown like d_pin:
    // positions [Nf][3], feature rows [Nf][pharm_nf]) and its level's coefficients.  seed_armed: the next begin starts from it;
    // taken off the handle on that begin's entry, dropped by a bind
    DevBuf d_seed;
    float *d_seed_x = nullptr, *d_seed_h = nullptr;
    float seed_alpha = 1.f, seed_sigma = 0.f, seed_feat_norm = 1.f;
    bool seed_armed = false;
    // multistep move (pf_denoise_step_ms): the previous step's outputs [Nf][3 + pharm_nf], written by the move itself (one
    // allocation, kept and grown like d_pin).  ms_hist_valid: the last move of the run in progress was a multistep move, so the
    // buffer holds that step's outputs; cleared by every begin, every bind and every other move
    DevBuf d_ms_hist;
    bool ms_hist_valid = false;
    // guided run (pf_sample_begin_guided): a pinned run plus restraint energies per graph.  restr: the restraint block (pf_restr.h),
    // packed at begin.  d_guide: what a guided step leaves (pf_restr.h: GuideWork), kept and grown like d_pin
    StagedBlock restr;
    int n_restr = 0;
    float guide_scale = 0.f, guide_clip = 0.f;
    DevBuf d_guide;
    bool guide_wide = true, guide_in_grads = false;   // the training family and the input-gradient switch the guided run began on
    bool guide_have = false;                // a guided step has run on this batch: pf_debug_last_guidance has something to return
    float* guide_traj_energy = nullptr;     // pf_sample_guided: row i of the caller's [n_steps][B] for the step in flight
    // pocket field (pf_guide_field_next): clash and complementarity energies next to a guided run's restraints.  Arming validates
    // and packs the caller's host arrays into the block's staging buffer in its layout (pf_field.h); the next pf_sample_begin_guided
    // uploads it, and the run's steps launch k_guide_field behind k_guide_grad.  armed: the next guided begin takes `arm`; on: the
    // run in progress uses `run`; have: the last guided step on this batch launched k_guide_field (pf_debug_last_field)
    struct FieldSource {
        StagedBlock blk; bool armed = false, on = false, have = false;
        struct Scalars { int n = 0; float w_clash = 0.f, w_comp = 0.f, kappa = 1.f, type_sharpness = 0.f; } arm, run;
    } field;
    // type guidance (pf_guide_types_next): typed restraints on the predicted clean feature rows, the complementarity energy's
    // feature gradient and the feature shift of the step end.  Armed, staged (pf_types.h) and uploaded like the pocket field.
    // d_tguide: what an armed step leaves (pf_restr.h: TypeWork).  have: the last guided step on this batch ran with type guidance
    // (pf_debug_last_type_guidance); live: that step's launches wrote g0_h / E_type (else they are zeros)
    struct TypesSource {
        StagedBlock blk;
        DevBuf d_tguide;
        bool armed = false, on = false, have = false, live = false;
        struct Scalars { int n = 0; float feat_scale = 0.f, feat_clip = 0.f, type_sharpness = 0.f; bool comp = false; float unmatched = 0.f; } arm, run;
    } types;
    // pair guidance (pf_guide_pairs_next): distance restraints between two centers of a graph.  Armed, staged (pf_pairs.h) and
    // uploaded like type guidance.  d_pguide: what a step with pair restraints leaves (pf_pairs.h: PairWork).  on: the run in
    // progress carries n_run > 0 pair restraints; have: the last guided step on this batch launched k_guide_pairs (pf_debug_last_pairs)
    struct PairsSource {
        StagedBlock blk;
        DevBuf d_pguide;
        bool armed = false, on = false, have = false;
        int n_arm = 0, n_run = 0;
    } pairs;
    // sample-set analysis (pf_sample_set_analyze): no run state -- the packed pointer block (pf_sset.h), the similarity matrices of a
    // call that passes no buffer for them, the status word and its pinned host copy.  Grown on demand, kept
    struct SsetWork {
        StagedBlock blk;
        DevBuf d_sim;
        DevArr<int32_t> d_status; PinnedArr<int32_t> status_host;
    } sset;
    // pharmacophore alignment (pf_pharm_align): no run state either -- the packed pointer block (pf_align.h), the self overlaps of
    // the call's queries and entries, the status word and its pinned host copy.  Grown on demand, kept
    struct AlignWork {
        StagedBlock blk;
        DevBuf d_self;
        DevArr<int32_t> d_status; PinnedArr<int32_t> status_host;
    } align;
    int max_np = 0, max_nf = 0;             // largest pocket of the batch, most centers in a graph
    bool edges_built = false;               // the dynamic edges of the current coordinates exist (built by k_step_build)
    bool edges_share = false;               // ... in the pocket-sharing form (no pa copies)
    // which form a launch takes (row-group quad streams, n16 streams: pk.rg_*, pk.n16_*): LaunchPolicy above
    // packed elements [pk.n16_begin, n_packed) are the n16 streams: no training kernel reads them, so pf_set_flat_params (called
    // after every optimiser step) refreshes only what precedes them and marks them stale; the first inference call afterwards
    // (run_dynamics without train, pf_debug_chain) gathers them (n16_refresh)
    bool n16_stale = false;
    // -DN16_SPLIT builds: the main quads of the n16 streams hold bf16 planes, two weights per 32-bit word -- not a gather (PackedModel::
    // split_tab); n16_refresh re-derives those words from the flat vector behind the gather (k_n16_split_words)
    DevArr<int4> d_split_tab; size_t n_split_tab = 0;
    bool tail_done = false;                 // the last run_dynamics call of a denoising step also did the step's update + build
    int last_tail = 0;                      // pf_debug_kernel_family(layer = n_convs): 0 / 4 (k_rg_tail) / 16 (k_n16_tail)
    float *d_msg_s2 = nullptr, *d_msg_v2 = nullptr;   // the last conv layer's message rows when conv layer 0's are still being read (fused launch)
    std::vector<int> last_family;           // per conv layer: pf_debug_kernel_family
    int last_hoist = 0;                     // pf_debug_l0_hoist
    // ---- static hoist of conv layer 0's pp messages (pf_rg.hip, EdgeParams::zs).  Everything derived from the weights
    // carries the version of the weights it was computed from (commit / pf_set_flat_params bump w_version).
    bool l0_hoist = true;                   // PFDYN_NO_L0_HOIST=1: off
    uint64_t w_version = 1, zs_version = 0, ptab_version = 0;
    bool l0_onehot = false;                 // every protein feature row of the batch is an element one-hot
    bool coords_custom = false;             // protein coordinates came from the caller of this call (not the batch's own)
    bool zs_batch_coords = false;           // d_zs was computed from (a rigid translate of) the batch's coordinates
    DevArr<float> d_l0c;                    // [32]
    DevArr<float> d_ptab;                   // [L0_PTAB_SLOTS][L0_NTAB][rec_nf][128] tables of the timesteps seen (scalar-t calls)
    std::unordered_map<uint32_t, int> ptab_slot;
    int *d_eorig = nullptr, *d_ptype = nullptr, *d_l0flag = nullptr;
    // edge records of the ff / pf slots (BuildParams::rec / FusedParams::rec): written by the merged launch's update + build for the next
    // call's fused launch; rec_valid: the edges in place are the ones that build emitted, with their records
    int4* d_rec = nullptr; bool rec_valid = false;
    float *d_zs = nullptr, *d_ptab_pg = nullptr;
    bool enc_on_the_fly = true;             // PFDYN_NO_ENC_FLY=1: always launch the encoders
    bool step_build_fast = true;            // PFDYN_NO_FAST_BUILD=1: the generic update + build bodies
    bool rg_compact = true;                 // PFDYN_NO_COMPACT=1: row-group edge launches walk the tile lists
    bool fuse_head = true;                  // last conv layer's node update + noise head in one launch (PFDYN_NO_FUSE_HEAD=1: separate)
    void init_tuning() {
        if (const char* e = getenv("PFDYN_NO_PRE")) use_pre = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_NO_FUSE_HEAD")) fuse_head = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_NO_PRUNE")) prune = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_NO_ENC_FLY")) enc_on_the_fly = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_NO_COMPACT")) rg_compact = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_NO_FAST_BUILD")) step_build_fast = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_NO_L0_HOIST")) l0_hoist = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_NO_CENTER_HOIST")) cen_hoist = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_NO_PA_SPEC")) pa_spec = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_PA_SPEC_SPLIT")) pa_spec_split = !strcmp(e, "mid") ? -1 : (!strcmp(e, "step") ? -2 : std::max(atoi(e), 0));
        if (const char* e = getenv("PFDYN_PA_CHECK")) pa_check = atoi(e) != 0;
        if (const char* e = getenv("PFDYN_NO_POCKET_SHARE")) share_disable = atoi(e) != 0;
        if (const char* e = getenv("PFDYN_TRAIN_TILE_NODE")) train_rg_node = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_TRAIN_TILE_EDGE")) train_rg_edge = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_TRAIN_TILE_HEAD")) train_rg_head = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_TRAIN_NODE_RECOMPUTE")) train_node_save = atoi(e) == 0;
        if (const char* e = getenv("PFDYN_TRAIN_BF16")) train_bf16 = atoi(e) != 0;
        if (const char* e = getenv("PFDYN_NO_FIX_FUSE")) no_fix_fuse = atoi(e) != 0;
        if (const char* e = getenv("PFDYN_VJP_FULL_KERNELS")) vjp_full_kernels = atoi(e) != 0;
        if (const char* e = getenv("PFDYN_NO_FIXED_SHAPES")) no_fixed_shapes = atoi(e) != 0;
        pol.from_env();
    }

    // ---- gradient path (pf_train_*): flat parameter vector in state-dict order, GvpT tables, per-layer activations
    DevArr<float> d_flat;
    size_t nparams = 0;
    FlatLayout flat_layout;                 // name -> (offset, numel), state-dict order
    DevArr<GvpT> d_gvpt;                    // same indexing as the GvpW table
    DevArr<int> d_map;                      // packed element -> flat parameter index (-1: zero): PackedModel::map
    size_t n_packed = 0;
    DevBuf d_tws;                           // training workspace of the current batch (allocated on first use, kept across batches like d_ws)
    std::vector<float*> t_H, t_V, t_msg_s, t_msg_v;
    std::vector<float*> t_sv_z, t_sv_g, t_sv_v;     // per layer: [n_message_gvps][Ecap] rows saved by the forward
    float *t_gs_buf = nullptr, *t_gv_buf = nullptr;
    int et_tile0[5] = {0, 0, 0, 0, 0};      // tile ranges of ff, pf, fp, pp in d_edge_tiles
    int et_tile0_act[5] = {0, 0, 0, 0, 0};  // ... of ff, pf, fp, pa in d_edge_tiles_act
    float *t_G_h[2] = {nullptr, nullptr}, *t_G_v[2] = {nullptr, nullptr}, *t_gagg_s = nullptr, *t_gagg_v = nullptr,
          *t_gpart = nullptr, *t_geps_h = nullptr, *t_geps_x = nullptr;
    long long *t_A_h = nullptr, *t_A_v = nullptr;      // fixed-point accumulators of the level-0 scatter (kept clear between uses)
    float* d_lpart = nullptr;               // k_loss_eval's arrival counter (first 64 bytes) + partial sums: in the workspace's zero section
    DevBuf d_tA;                            // their own allocation: it outlives the batches, so "kept clear" holds across them
    bool tA_dirty = false;                  // a backward pass stopped between the scatter and pfk_fix_apply
    int enc_begin = 0, enc_n = 0;           // flat range of the encoders' parameters (contiguous: the first tensors of the state dict)
    float* t_gpart_enc = nullptr;
    DevArr<TensorSeg> d_tseg; int n_tseg = 0;   // class of every parameter tensor (pf_train.h: which gradient copies hold it)
    int n_gvpt = 0;                         // entries of d_gvpt (message, update, head GVPs)
    DevArr<float> d_wpack;                  // k_pack_gvp tables of every GVP (input-gradient fragments, then forward fragments); valid for w_version == wpack_version
    uint64_t wpack_version = ~0ull;
    float *t_lx0c = nullptr, *t_lag = nullptr, *t_lsg = nullptr, *t_lcom2 = nullptr, *t_lgx = nullptr, *t_lgh = nullptr, *t_lout = nullptr;   // pf_train_loss_forward
    bool t_have_loss = false;
    float* t_Gg = nullptr;                  // encoder backward: upstream gradient summed per (graph, element)
    int* t_ulist = nullptr;                 // dense per-type row list of the layer being differentiated (k_compact_node_rows; counts: t_ccnt[97], [98])
    int t_ucap = 0;
    size_t t_clist_cap = 0, t_ulist_cap = 0;   // ints per conv layer in t_clist / t_ulist (one list per layer: they are built ahead, on the side stream)
    int *t_clist = nullptr, *t_ccnt = nullptr;   // dense list of the valid edge slots of the layer being differentiated (k_compact_rows), counts
    float* t_fix = nullptr;                 // [2] scale / inverse scale of the current backward call
    int t_nblk = 0;
    const float* t_mask_override = nullptr; // pf_debug_set_dropout_masks
    bool t_have_fwd = false;
    bool t_ws_ready = false;                // d_tws is carved (and its zero rows set) for the current batch
    // pf_train_set_family: the width-generic training leg (pf_wide.hip's training form, pf_wide_train.hip) and its workspace --
    // like d_tws one allocation that outlives the batch, carved again for every new batch (ensure_wide_train_ws)
    bool train_wide = false;
    // pf_train_set_input_grads: the tuned family's fp32 backward also gives dL/d(center coordinates, feature rows).  The switch owns
    // d_gdiff, the per-edge dL/d(x_src - x_dst) rows [n_convs][max(Ecap, 1)][3] of a pass's level-0 launches: cleared per pass, kept
    // and grown like a run's scratch (reserve behind Wait::on(the caller's stream)), released when the switch goes off
    bool train_in_grads = false;
    DevBuf d_gdiff;
    // pf_adam_step_guarded / pf_debug_optim_step: one fp64 partial per chunk of the gradient (grown on demand, kept)
    DevArr<double> d_optim_part;
    // a handle of the specialised widths carries no width-generic packing (inference stays on the tuned kernels): its wide training
    // leg builds the WideGvp table on first use (ensure_wide_pack) -- Wh, Wu and the biases read from d_flat as stored, to_feats_out
    // and the gate Linear packed on the device into d_wpk whenever w_version moved
    DevArr<float> d_wpk; DevArr<WidePackJob> d_wpk_jobs; int n_wpk_jobs = 0; uint64_t wpk_version = ~0ull;
    DevBuf d_wtws; bool wt_ready = false;
    DevBuf d_wtA;                           // the fixed-point accumulators [N][S], [N][V][3] (int64), zero between passes
    struct WtWs {
        float *esv_s, *esv_v;               // per conv layer [n_message_gvps][Ecap] level inputs of the message chains
        float *x1_s, *x1_v, *x2_s, *x2_v;   // per conv layer [N] rows in front of the two GVPLayerNorms
        float *usv_s, *usv_v;               // per conv layer [n_update_gvps][N] level inputs of the update chains
        float *hsv_s, *hsv_v, *h64;         // [n_noise_gvps][Nf] level inputs of the head, its 64 output scalars [Nf]
        float *G_s[2], *G_v[2];             // dL/d(layer output / input), ping-pong [N]
        float *gch_s, *gch_v, *gres_s, *gres_v, *gagg_s, *gagg_v;   // per node: chain gradient, residual branch, aggregate
        float *ges, *gev;                   // per edge slot: gradient between two message-chain levels
        float *xkeep, *gdiff;               // input gradients: the coordinates the forward read (float4 [N]); per conv layer and
                                            // edge slot dL/d(x_src - x_dst) [Ecap][3]
        float *gpart, *fix;
        float *st_h[2], *st_v[2], *msg_s, *msg_v;   // the training forward's own layer states [N] and message rows [Ecap]: the
                                                    // inference buffers (and what the tuned kernels expect in them) stay untouched
        long long *A_h, *A_v;
        size_t Es;
    } wt{};
    WtCommon wt_common{};
    TrainCommon t_common{};
    // offsets into the flat vector that every training call reads, resolved by name once per commit (pf_pack.h: param_offsets) --
    // the training step is host-bound with a new batch every step, and looking ~26 names up per backward pass was 50-100 us of it
    ParamOffsets po;
    unsigned prof_mask = 0;                 // pf_profile_*: which classes are timed, and how many of prof_ev's pairs this window used
    size_t prof_used[K_NUM] = {};
};

namespace {

#define PF_FAIL(h, code, ...)                                   \
    do {                                                        \
        char _b[512];                                           \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                  \
        (h)->err = _b;                                          \
        return (code);                                          \
    } while (0)

#define PF_HIP(h, call)                                                                              \
    do {                                                                                             \
        hipError_t _e = (call);                                                                      \
        if (_e != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(_e)); \
    } while (0)

// Replaces the device buffer with a copy of v (an empty v leaves it empty).
template <typename T>
static hipError_t upload(DevArr<T>& buf, const std::vector<T>& v) {
    buf.release();
    if (v.empty()) return hipSuccess;
    const hipError_t e = buf.reserve(v.size() * sizeof(T), v.size() * sizeof(T), Wait::none());
    return e != hipSuccess ? e : hipMemcpy(buf, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// keep_ws: the inference workspace stays allocated (pf_set_pocket_batch re-carves it when the next batch fits: a
// free / allocate pair of a few hundred MB per batch costs milliseconds)
static void free_ws(pf_handle* h, bool keep_ws = false) {
    if (h->d_ws && !keep_ws) { h->d_ws.release(); h->d_xchg = nullptr; h->d_lpart = nullptr; h->d_xchg2 = nullptr; h->d_cen_h = h->d_cen_p = nullptr; h->d_snap[0] = h->d_snap[1] = nullptr; h->d_pa_stamp = h->d_pa_same = nullptr; h->d_pa_cnt = h->d_pa_gstamp = nullptr; }
    if (!keep_ws) for (DevBuf* b : {&h->d_tws, &h->d_tA, &h->d_wtws, &h->d_wtA}) b->release();
    h->t_ws_ready = false;
    h->wt_ready = false;
    h->t_have_fwd = false;
    h->t_mask_override = nullptr;
    h->have_batch = false;
}

template <typename T>
static T* carve(char*& cur, size_t count) {
    T* p = reinterpret_cast<T*>(cur);
    size_t bytes = count * sizeof(T);
    bytes = (bytes + 255) & ~size_t(255);
    cur += bytes;
    return p;
}

// One list for sizes and pointers: a workspace's buffers are one sequence of take() calls that runs twice -- first over a
// dummy base, which only counts the bytes, then over the allocation, which hands the pointers out
struct Carver {
    char* const base;
    char* cur;
    const bool assign;
    explicit Carver(void* allocation) : base(allocation ? static_cast<char*>(allocation) : reinterpret_cast<char*>(uintptr_t(256))), cur(base), assign(allocation != nullptr) {}
    template <typename T>
    void take(T*& dst, size_t n) { T* q = carve<T>(cur, n); if (assign) dst = q; }
    size_t bytes() const { return (size_t)(cur - base); }
};

struct ProfScope {
    pf_handle* h; int k; hipStream_t s; bool on;
    ProfScope(pf_handle* h_, int k_, hipStream_t s_) : h(h_), k(k_), s(s_), on((h_->prof_mask >> k_) & 1u) {
        if (!on) return;
        if (h->prof_used[k] == h->prof_ev[k].size()) h->prof_ev[k].emplace_back(Event(true), Event(true));   // (timing events)
        if (h->prof_ev[k][h->prof_used[k]].first.record(s) != hipSuccess) on = false;
    }
    ~ProfScope() {
        if (!on) return;
        (void)h->prof_ev[k][h->prof_used[k]].second.record(s);
        h->prof_used[k]++;
    }
};

static bool l0_hoist_ok(pf_handle* h);
// the conv layer restricted to active atoms (receptive-field pruning of the second-to-last layer); -1: none
static int prune_layer(const pf_handle* h) { return (h->prune && h->cfg.n_convs >= 2) ? h->cfg.n_convs - 2 : -1; }
// Which tiles a conv layer walks, forward and backward.  The last layer's output is read on the centers only: their node tiles
// and the ff / pf edge tiles (the head of either table).  The pruned layer walks the active atoms' tables.  Every other layer,
// everything.
struct LayerTiles {
    const EdgeTile* etiles; int n_etiles;
    const int* et_tile0; int n_et;          // etype segments of the edge table [5]; etypes [0, n_et) take part in the gradient
    const NodeTile* ntiles; int n_ntiles;
    int pp_slot;                            // in_cnt slot of the pp edges (2: the active atoms' compact copy)
};
static LayerTiles layer_tiles(const pf_handle* h, bool last, bool pruned) {
    LayerTiles t;
    t.etiles = pruned ? h->d_edge_tiles_act : h->d_edge_tiles;
    t.n_etiles = last ? h->n_edge_tiles_last : (pruned ? h->n_edge_tiles_act : h->n_edge_tiles);
    t.et_tile0 = pruned ? h->et_tile0_act : h->et_tile0;
    t.n_et = last ? 2 : 4;                  // the last layer's fp / pp messages reach no output
    t.ntiles = pruned ? h->d_node_tiles_act : h->d_node_tiles;
    t.n_ntiles = last ? h->n_node_tiles_last : (pruned ? h->n_node_tiles_act : h->n_node_tiles);
    t.pp_slot = pruned ? 2 : 1;
    return t;
}
static LayerTiles layer_tiles(const pf_handle* h, int l) { return layer_tiles(h, l == h->cfg.n_convs - 1, l == prune_layer(h)); }
// pocket sharing applies to inference calls at one common t whose conv layer 0 is the pruned layer under the static hoist
static bool share_now(pf_handle* h) {
    const pf_config& c = h->cfg;
    if (h->share_ok && h->share_check == 0) {        // device rows: the comparison's verdict arrived with the one-hot flag
        (void)h->l0flag_ev.sync();
        h->share_check = (h->l0flag_host && h->l0flag_host[1] == 0) ? 1 : 2;
    }
    if (h->share_check == 2) return false;           // (run_dynamics fails the call: a false claim is the caller's bug, not a mode)
    return !h->wide && h->share_ok && !h->share_disable && h->prune && c.n_convs == 2 && h->rg_compact && l0_hoist_ok(h);
}
// what the next denoising step's dynamics call will ask for (the mode its edges are built in)
static bool share_next(pf_handle* h) { return (h->prune && h->cfg.n_convs == 2) && share_now(h); }
// the fast update + build's shape (one atom per thread, the latency-optimised kernel): kNN pf edges, pockets of at most 512 atoms
static bool step_build_fast_ok(const pf_handle* h) { return h->cfg.pf_k > 0 && h->max_np <= 512 && h->cfg.pharm_nf <= 16 && h->step_build_fast; }
// a build with these parameters has been enqueued: its stamp is what the next shared edge launch looks for
static void build_done(pf_handle* h, bool share, bool with_records = false) {
    h->rec_valid = with_records;
    h->edges_share = share;
    if (share) h->edges_stamp = ++h->need_stamp;
}
static BuildParams build_params(pf_handle* h, bool share = false) {
    const pf_config& c = h->cfg;
    BuildParams bp{};
    bp.B = h->B; bp.Np_tot = h->Np;
    bp.prot_ptr = h->d_prot_ptr; bp.pharm_ptr = h->d_pharm_ptr; bp.xn = h->d_xn;
    bp.reg = h->d_reg; bp.dyn_cnt = h->d_dyn_cnt; bp.esrc = h->d_esrc; bp.edst = h->d_edst;
    bp.in_start = h->d_in_start; bp.in_cnt = h->d_in_cnt; bp.N = h->N;
    bp.ff_k = c.ff_k; bp.pf_k = c.pf_k;
    bp.r2_ff = c.cutoff_ff * c.cutoff_ff; bp.r2_pf = c.cutoff_pf * c.cutoff_pf;
    bp.gnorm = h->d_gnorm; bp.pp_cnt = h->d_pp_cnt; bp.pfq_cnt = h->d_pfq_cnt; bp.norm_mode = c.message_norm_mode;
    if (h->pa_spec && h->run != RUN_NONE && h->d_pa_stamp && !share) { bp.pa_stamp = h->d_pa_stamp; bp.step_id = h->step_id; bp.pa_same = h->d_pa_same; }
    bp.act_ids = prune_layer(h) >= 0 ? h->d_act_ids : nullptr; bp.reg_act = h->d_reg_act;
    bp.eorig = h->d_eorig;
    bp.pa_static = share ? h->d_pa_static : nullptr;
    if (share) { bp.rep_base = h->d_rep_base; bp.need = h->d_need; bp.need_stamp = h->need_stamp + 1; }   // committed by build_done()
    return bp;
}
// ---- one builder per parameter struct (what does not depend on the call's mode; callers add the rest), one predicate per gate ----
// RBF centres (torch.linspace(0, dmax, dim)) and width of the edge distance embedding; returns sigma
static float rbf_params(const pf_config& c, float* mu, float* inv_sigma) {
    linspace_f32(0.f, c.rbf_dmax, c.rbf_dim, mu);
    const float sigma = (c.rbf_dmax - 0.f) / (float)c.rbf_dim;
    if (inv_sigma) *inv_sigma = 1.0f / sigma;
    return sigma;
}
static EncodeParams encode_params(const pf_handle* h, const float* t_scalar, float* h_out) {
    const pf_config& c = h->cfg;
    EncodeParams ep{};
    ep.Np = h->Np; ep.Nf = h->Nf; ep.rec_nf = c.rec_nf; ep.pharm_nf = c.pharm_nf;
    ep.prot_h0 = h->d_prot_h0; ep.pharm_h = h->d_pharm_h; ep.gid = h->d_gid; ep.h_out = h_out;
    ep.t = t_scalar ? nullptr : h->d_t; ep.t_scalar = t_scalar ? *t_scalar : 0.f;
    for (int nt = 0; nt < 2; ++nt) {
        ep.w[nt] = h->d_w + h->pk.enc_w[nt]; ep.b[nt] = h->d_w + h->pk.enc_b[nt];
        ep.ln_w[nt] = h->d_w + h->pk.enc_lw[nt]; ep.ln_b[nt] = h->d_w + h->pk.enc_lb[nt];
    }
    return ep;
}
// the noise head; h / v (a launch of its own reads the last layer's output) and the exchange words (merged launch) are the caller's
static HeadParams head_params(const pf_handle* h, float* eps_h, float* eps_x) {
    const pf_config& c = h->cfg;
    HeadParams hp{};
    hp.tiles = h->d_head_tiles; hp.ntiles = h->n_head_tiles; hp.node_base = h->Np;
    hp.gvps = h->d_gvp + h->head_base(); hp.n_gvps = c.n_noise_gvps;
    hp.a_out = h->d_w + h->pk.out_a; hp.b_out = h->d_w + h->pk.out_b; hp.pharm_nf = c.pharm_nf; hp.eps_h = eps_h; hp.eps_x = eps_x;
    return hp;
}
// edge messages of a conv layer: tiles, geometry, GVP table, RBF, the row-group streams.  The caller's: h / v / msg rows, regions,
// the hoist's and the n16 form's fields, the two-wave streams (rgs: pf_debug_conv_layer passes none)
static EdgeParams edge_params_base(const pf_handle* h, int layer, bool last, bool pruned) {
    const pf_config& c = h->cfg;
    const LayerTiles lt = layer_tiles(h, last, pruned);
    EdgeParams e{};
    e.tiles = lt.etiles; e.ntiles = lt.n_etiles; e.dyn_cnt = h->d_dyn_cnt;
    e.esrc = h->d_esrc; e.edst = h->d_edst; e.xn = h->d_xn;
    e.w = h->d_gvp + h->msg_base(layer, 0); e.n_gvps = c.n_message_gvps;
    rbf_params(c, e.rbf_mu, &e.rbf_inv_sigma);
    for (int et = 0; et < 4; ++et) e.rg[et] = h->d_w + h->pk.rg_msg[(size_t)layer * 4 + et];
    return e;
}
// node update of a conv layer.  The caller's: msg rows, h / v in and out, grp / grp_pa, pp_slot 3 of a shared launch, the two-wave streams
static NodeParams node_params_base(const pf_handle* h, int layer, bool last, bool pruned) {
    const pf_config& c = h->cfg;
    const LayerTiles lt = layer_tiles(h, last, pruned);
    NodeParams n{};
    n.tiles = lt.ntiles; n.ntiles = lt.n_ntiles;
    n.in_start = h->d_in_start; n.in_cnt = h->d_in_cnt; n.N = h->N;
    n.pp_slot = lt.pp_slot; n.row_ids = h->d_act_ids; n.dyn_cnt = h->d_dyn_cnt; n.zero_row = h->zero_row;
    n.gid = h->d_gid; n.gnorm = h->d_gnorm; n.B = h->B; n.norm_mode = c.message_norm_mode; n.norm_value = c.message_norm_value;
    n.n_upd = c.n_update_gvps;
    for (int nt = 0; nt < 2; ++nt) {
        const size_t* lo = &h->pk.ln_off[(size_t)(layer * 2 + nt) * 4];
        n.w[nt].ln1_w = h->d_w + lo[0]; n.w[nt].ln1_b = h->d_w + lo[1];
        n.w[nt].ln2_w = h->d_w + lo[2]; n.w[nt].ln2_b = h->d_w + lo[3];
        n.w[nt].upd = h->d_gvp + h->upd_base(layer, nt);
        n.rg_upd[nt] = h->d_w + h->pk.rg_upd[(size_t)layer * 2 + nt];
    }
    return n;
}
// the "pa" rows of this conv-layer-0 launch may be computed ahead (k_n16_pa_spec): one contract for the side that saves the launch's
// parameters for the speculative items and the side that skips the regions they filled
static bool pa_ahead_ok(const pf_handle* h, const EdgeParams& e, bool shared) { return h->pa_spec && !shared && h->B <= 64 && !e.need; }
// the timestep behind t in the announced plan (searched from plan_pos on); NaN when nothing follows.  index (optional): where t was found
static float planned_next_t(const pf_handle* h, float t, size_t* index) {
    const size_t n = h->t_plan.size();
    for (size_t k = 0; k < n; ++k) {
        const size_t i = (h->plan_pos + k) % n;
        if (h->t_plan[i] != t) continue;
        if (index) *index = i;
        return i + 1 < n ? h->t_plan[i + 1] : NAN;
    }
    return NAN;
}
// every graph has regions of one capacity at a fixed stride, for each of the first n_et edge types: the item map of a launch
// can be arithmetic.  The strides fit 16 bits (both users pack them so); what the capacities must fit is the caller's
static bool uniform_regions(const pf_handle* h, int n_et, int* stride, int* cap) {
    for (int et = 0; et < n_et; ++et) {
        const size_t o = (size_t)et * h->B;
        stride[et] = h->B > 1 ? h->h_reg[o + 1] - h->h_reg[o] : 0; cap[et] = h->h_cap[o];
        for (int g = 0; g < h->B; ++g)
            if (h->h_cap[o + g] != cap[et] || h->h_reg[o + g] != h->h_reg[o] + g * stride[et]) return false;
        if (stride[et] < 0 || stride[et] >= 65536) return false;
    }
    return true;
}
// profile class of an edge launch on the latency-regime forms: the last of several conv layers is timed apart
static int edge_prof_class(bool last, int n_convs) { return (last && n_convs > 1) ? pf_handle::K_EDGE_LAST : pf_handle::K_EDGE_COOP; }
// conv layer 0 of an inference call runs on the row-group kernels: they encode the rows they read on the fly, so the
// call's first launch is the edge build alone -- which the previous denoising step's update launch can do as well
static bool encoders_on_the_fly(const pf_handle* h) {
    if (h->wide) return false;          // (the width-generic family launches its encoders; pf_denoise_step: the update alone)
    const pf_config& c = h->cfg;
    const int nt0 = c.n_convs == 1 ? h->n_edge_tiles_last : (prune_layer(h) == 0 ? h->n_edge_tiles_act : h->n_edge_tiles);
    return h->enc_on_the_fly && h->pol.rg_mode(nt0) != 0;
}

// ---- static hoist of conv layer 0 (pf_rg.hip: EdgeParams::zs) ----------------------------------------------------
// usable for this handle / batch at all (inference, row-group kernels with encoders on the fly)
// The device-side one-hot check of pf_set_pocket_batch is read back lazily: only an inference call that could use the
// static hoist waits for it (callers that pass the element types themselves never wait).
static void l0_resolve_onehot(pf_handle* h) {
    if (h->l0_state != 0) return;
    (void)h->l0flag_ev.sync();
    h->l0_state = (h->Np > 0 && h->l0flag_host && *h->l0flag_host == 0) ? 1 : 2;
    h->l0_onehot = h->l0_state == 1;
}
static bool l0_hoist_ok(pf_handle* h) {
    if (h->l0_hoist && h->l0_state == 0) l0_resolve_onehot(h);
    const pf_config& c = h->cfg;
    return h->l0_hoist && h->l0_onehot && h->Epp > 0 && c.n_message_gvps >= 2 && c.rbf_dim == PF_R && c.rec_nf < 128 &&
           encoders_on_the_fly(h);
}
static L0HoistParams l0_params(pf_handle* h) {
    const pf_config& c = h->cfg;
    L0HoistParams lp{};
    lp.src = h->d_w + h->pk.l0h_off; lp.l0c = h->d_l0c;
    lp.esrc = h->d_esrc; lp.edst = h->d_edst; lp.xn = h->d_xn; lp.Epp = (int)h->Epp; lp.zs = h->d_zs;
    float mu[PF_R];
    rbf_params(c, mu, &lp.rbf_inv_sigma);
    lp.rbf_mu0 = mu[0]; lp.rbf_mu_step = (mu[PF_R - 1] - mu[0]) * (1.0f / (float)(PF_R - 1));
    lp.enc_w = h->d_w + h->pk.enc_w[0]; lp.enc_b = h->d_w + h->pk.enc_b[0];
    lp.enc_lw = h->d_w + h->pk.enc_lw[0]; lp.enc_lb = h->d_w + h->pk.enc_lb[0];
    lp.rec_nf = c.rec_nf;
    return lp;
}
// the trajectory constants (zs, weff) of the current protein coordinates and weights
static void l0_ensure_static(pf_handle* h, hipStream_t s) {
    if (!h->coords_custom && h->zs_batch_coords && h->zs_version == h->w_version) return;
    const L0HoistParams lp = l0_params(h);
    pfk_l0_hoist(&lp, 0, s);
    h->zs_version = h->w_version;
    h->zs_batch_coords = !h->coords_custom;
}
// type tables of n timesteps (scalar-t calls): slots of the resident cache, computed on a miss
static void l0_prepare_t(pf_handle* h, const float* tv, int n, hipStream_t s) {
    if (h->ptab_version != h->w_version) { h->ptab_slot.clear(); h->ptab_version = h->w_version; }
    const size_t slot_floats = (size_t)L0_NTAB * h->cfg.rec_nf * PF_S;
    int i = 0;
    while (i < n) {
        L0HoistParams lp = l0_params(h);
        if (h->ptab_slot.size() + 64 > L0_PTAB_SLOTS) h->ptab_slot.clear();     // stream order keeps earlier launches valid
        const int slot0 = (int)h->ptab_slot.size();
        int m = 0;
        for (; i < n && m < 64; ++i) {
            uint32_t bits; memcpy(&bits, &tv[i], 4);
            if (h->ptab_slot.count(bits)) continue;
            h->ptab_slot[bits] = slot0 + m;
            lp.t_host[m++] = tv[i];
        }
        if (m == 0) continue;
        lp.nt = m; lp.t_dev = nullptr; lp.ptab = h->d_ptab + (size_t)slot0 * slot_floats;
        pfk_l0_hoist(&lp, 1, s);
    }
}

// the n16 streams after pf_set_flat_params left them behind (see pf_handle::n16_begin)
static void n16_refresh(pf_handle* h, hipStream_t s) {
    if (!h->n16_stale) return;
    pfk_gather_weights(h->d_flat, h->d_map + h->pk.n16_begin, h->n_packed - h->pk.n16_begin, h->d_w + h->pk.n16_begin, s);
    if (h->n_split_tab) pfk_n16_split_words(h->d_flat, h->d_split_tab, h->n_split_tab, h->d_w, s);     // (-DN16_SPLIT: the bf16-plane words)
    h->n16_stale = false;
}

// The WideGvp table of a handle that was not created on the width-generic family (the specialised widths without PFDYN_WIDE), for
// its wide training leg: Wh, Wu and the biases point into the flat parameter vector, which stores them in the layout the kernels
// read; to_feats_out and the gate Linear of every GVP sit in fragment order in d_wpk, written from the flat vector by k_wide_pack
// (ensure_wide_pack).  A handle of the family itself has the table from pf_commit_weights and the gather map keeps it fresh.
static int ensure_wide_pack(pf_handle* h, hipStream_t s) {
    if (h->wide) return PF_OK;
    const pf_config& c = h->cfg;
    if (!h->d_wgvp) {
        std::vector<WideGvp> tab;
        std::vector<WidePackJob> jobs;
        size_t total = 0;
        auto frag = [](int n_out, int K) { return (size_t)((n_out + 15) / 16) * ((K + 3) / 4) * 64; };
        for_each_gvp(c, [&](const GvpSpec& g) {
            const int H = std::max(g.vi, g.vo);
            const int* o = &h->po.gvp[6 * tab.size()];     // Wh Wu Wm bm Wg bg
            WideGvp w{};                    // (wm, wg: below, once d_wpk exists)
            w.wh = h->d_flat + o[0]; w.wu = h->d_flat + o[1]; w.bm = h->d_flat + o[3]; w.bg = h->d_flat + o[5];
            w.vi = g.vi; w.vo = g.vo; w.si = g.si; w.so = g.so;
            jobs.push_back({o[2], g.so, g.si + H, (int)total});
            total += frag(g.so, g.si + H);
            jobs.push_back({o[4], g.vo, g.so, (int)total});
            total += frag(g.vo, g.so);
            tab.push_back(w);
        });
        if (total >= (size_t)1 << 31) PF_FAIL(h, PF_ERR_ARG, "pf_train_set_family: the model is too large for the width-generic packing");
        h->d_wpk.release();
        PF_HIP(h, h->d_wpk.reserve(std::max<size_t>(total, 1) * sizeof(float), std::max<size_t>(total, 1) * sizeof(float), Wait::none()));
        PF_HIP(h, upload(h->d_wpk_jobs, jobs));
        h->n_wpk_jobs = (int)jobs.size();
        for (size_t i = 0; i < tab.size(); ++i) { tab[i].wm = h->d_wpk + jobs[2 * i].dst; tab[i].wg = h->d_wpk + jobs[2 * i + 1].dst; }
        PF_HIP(h, upload(h->d_wgvp, tab));
        h->wpk_version = ~0ull;
    }
    if (h->wpk_version != h->w_version) {
        pfk_wide_pack(h->d_flat, h->d_wpk_jobs, h->n_wpk_jobs, h->d_wpk, s);
        h->wpk_version = h->w_version;
    }
    return PF_OK;
}

// One dynamics call on the width-generic family (pf_wide.hip): encoders, the edge build, per conv layer one message launch and
// one node launch (the last one with the noise head).  The same tile lists as the specialised path: the last layer computes the
// ff / pf messages and the centers only, the layer before it (receptive-field pruning) the active atoms and the centers.
// train: the training form (pf_train_set_family) -- dropout, and what the gradient kernels read again goes to h->wt
static int run_dynamics_wide(pf_handle* h, float* eps_h, float* eps_x, hipStream_t s, const float* t_scalar, bool train = false) {
    const pf_config& c = h->cfg;
    h->tail_done = false; h->last_tail = 0; h->last_hoist = 0;
    h->cen_valid = false; h->last_cen = false; h->spec_valid = false; h->last_spec = 0; h->last_forms = 0; h->e0_saved = false;
    // a pocket-group claim is verified as on the specialised path; the family then computes every graph itself
    if (!train && h->share_ok && h->share_check == 0) (void)share_now(h);
    if (!train && h->share_check == 2)
        PF_FAIL(h, PF_ERR_ARG, "pf_set_pocket_groups: the claim made for this batch is false -- a graph differs from its representative in "
                               "coordinates or features (compared on the device); bind the batch again without the claim");
    const int rc = ensure_wide_pack(h, s);
    if (rc) return rc;
    const int S = c.n_hidden_scalars, V = c.vector_size;
    WideEncParams ep{};
    ep.Np = h->Np; ep.Nf = h->Nf; ep.S = S; ep.rec_nf = c.rec_nf; ep.pharm_nf = c.pharm_nf;
    ep.prot_h0 = h->d_prot_h0; ep.pharm_h = h->d_pharm_h;
    ep.t = t_scalar ? nullptr : h->d_t; ep.t_scalar = t_scalar ? *t_scalar : 0.f; ep.gid = h->d_gid;
    for (int nt = 0; nt < 2; ++nt) {
        ep.w[nt] = h->d_w + h->pk.enc_w[nt]; ep.b[nt] = h->d_w + h->pk.enc_b[nt];
        ep.ln_w[nt] = h->d_w + h->pk.enc_lw[nt]; ep.ln_b[nt] = h->d_w + h->pk.enc_lb[nt];
    }
    float* const* st_h = train ? h->wt.st_h : h->d_h;
    float* const* st_v = train ? h->wt.st_v : h->d_v;
    ep.h_out = st_h[0];
    { ProfScope ps(h, pf_handle::K_ENCODE, s); pfk_wide_encode(&ep, s); }
    if (!h->edges_built) {
        const BuildParams bp = build_params(h, false);
        { ProfScope ps(h, pf_handle::K_BUILD, s); pfk_build_edges(&bp, s); }
        build_done(h, false);
    }
    h->last_family.assign(c.n_convs, 64);
    // the gradient of the edge geometry reads the coordinates again (pf_train_backward_inputs): xn moves with the next call
    if (train) pfk_copy(reinterpret_cast<const float*>(h->d_xn), h->wt.xkeep, (size_t)h->N * 4, s);
    int cur = 0;
    for (int l = 0; l < c.n_convs; ++l) {
        const bool last = l == c.n_convs - 1;
        const LayerTiles lt = layer_tiles(h, l);
        WideEdgeParams e{};
        e.tiles = lt.etiles; e.ntiles = lt.n_etiles;
        e.dyn_cnt = h->d_dyn_cnt; e.esrc = h->d_esrc; e.edst = h->d_edst; e.xn = h->d_xn;
        e.h = st_h[cur]; e.v = st_v[cur]; e.layer0 = l == 0;
        e.msg_s = train ? h->wt.msg_s : h->d_msg_s; e.msg_v = train ? h->wt.msg_v : h->d_msg_v;
        e.w = h->d_wgvp + h->msg_base(l, 0); e.n_gvps = c.n_message_gvps; e.S = S; e.V = V;
        e.rbf_sigma = rbf_params(c, e.rbf_mu, nullptr);
        const size_t N_ = (size_t)h->N, V3_ = (size_t)3 * V;
        if (train) {
            const size_t nm = (size_t)c.n_message_gvps;
            e.sv_rows = h->wt.Es;
            e.sv_s = h->wt.esv_s + (size_t)l * nm * h->wt.Es * (S + PF_R); e.sv_v = h->wt.esv_v + (size_t)l * nm * h->wt.Es * 3 * (V + 1);
        }
        { ProfScope ps(h, pf_handle::K_EDGE, s); pfk_wide_edge(&e, train ? 1 : 0, s); }
        WideNodeParams n{};
        n.tiles = lt.ntiles; n.ntiles = lt.n_ntiles;
        n.dyn_cnt = h->d_dyn_cnt; n.row_ids = h->d_act_ids;
        n.in_start = h->d_in_start; n.in_cnt = h->d_in_cnt; n.N = h->N; n.pp_slot = lt.pp_slot;
        n.msg_s = e.msg_s; n.msg_v = e.msg_v;
        n.h_in = e.h; n.v_in = e.v; n.layer0 = e.layer0;
        n.h_out = st_h[cur ^ 1]; n.v_out = st_v[cur ^ 1];
        n.gid = h->d_gid; n.gnorm = h->d_gnorm; n.B = h->B; n.norm_mode = c.message_norm_mode; n.norm_value = c.message_norm_value;
        for (int nt = 0; nt < 2; ++nt) {
            const size_t* lo = &h->pk.ln_off[(size_t)(l * 2 + nt) * 4];
            n.ln1_w[nt] = h->d_w + lo[0]; n.ln1_b[nt] = h->d_w + lo[1];
            n.ln2_w[nt] = h->d_w + lo[2]; n.ln2_b[nt] = h->d_w + lo[3];
            n.upd[nt] = h->d_wgvp + h->upd_base(l, nt);
        }
        n.n_upd = c.n_update_gvps; n.S = S; n.V = V;
        if (train) {
            const WtCommon& wc = h->wt_common;
            n.drop_thr = wc.drop_thr; n.seed = wc.seed; n.drop_scale = wc.drop_scale; n.mask_override = wc.mask_override; n.layer = l;
            n.x1_s = h->wt.x1_s + l * N_ * S; n.x1_v = h->wt.x1_v + l * N_ * V3_;
            n.x2_s = h->wt.x2_s + l * N_ * S; n.x2_v = h->wt.x2_v + l * N_ * V3_;
            n.sv_rows = N_;
            n.sv_s = h->wt.usv_s + l * c.n_update_gvps * N_ * S; n.sv_v = h->wt.usv_v + l * c.n_update_gvps * N_ * V3_;
            n.hsv_rows = (size_t)std::max(h->Nf, 1); n.hsv_s = h->wt.hsv_s; n.hsv_v = h->wt.hsv_v; n.h64 = h->wt.h64;
        }
        if (last) {             // the last layer's node tiles are the centers: the noise head follows in the same launch
            n.head = h->d_wgvp + h->head_base(); n.n_head = c.n_noise_gvps;
            // (a handle of the specialised widths on the wide training leg: to_scalar_output as the flat vector stores it)
            n.w_out = h->wide ? h->d_w + h->pk.wide_out_w : h->d_flat + h->po.out_w;
            n.b_out = h->wide ? h->d_w + h->pk.wide_out_b : h->d_flat + h->po.out_b;
            n.pharm_nf = c.pharm_nf; n.node_base = h->Np;
            n.eps_h = eps_h; n.eps_x = eps_x;
            ProfScope ps(h, pf_handle::K_HEAD, s); pfk_wide_node(&n, train ? 1 : 0, s);
        } else { ProfScope ps(h, pf_handle::K_NODE, s); pfk_wide_node(&n, train ? 1 : 0, s); }
        cur ^= 1;
    }
    h->edges_built = false;                 // whoever moves the coordinates next rebuilds
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(err));
    return PF_OK;
}

// ---- one dynamics call on the specialised kernels: the sequencer ------------------------------------------------------
// What is computed once per call and read by every piece below (a plain struct on run_dynamics' stack), and what one conv
// layer's edge launch hands to its node launch
struct DynCall {
    pf_handle* h; hipStream_t s; float *eps_h, *eps_x;
    const float* t_scalar; bool train; const StepParams* step;
    bool cen_have, spec_have;               // the previous step left the center hoist's tables / the "pa" rows for THIS call's timestep
    bool enc_fly, share, pre_ready, hoist, n16_batch, n16_l0, fuse_l0node;
    const float* l0_ptab; int l0_gstride, cur; bool head_done; EncodeParams ep; FusedParams fz;
    EdgeParams e; bool last, pruned, shared; int rg, rgp;       // the conv layer in flight
};
// capacity of the regions [r0, r1) in groups of gs slots (a shared kind-3 region is cut on absolute multiples of gs)
static int region_groups(const pf_handle* h, bool shared, int r0, int r1, int gs) {
    int n = 0;
    for (int r = r0; r < r1; ++r) {
        if (shared && r >= 3 * h->B) {
            const int st = h->h_share_start[r - 3 * h->B], cn = h->h_share_cnt[r - 3 * h->B];
            n += cn > 0 ? (st + cn - 1) / gs - st / gs + 1 : 0;
        } else n += (h->h_cap[r] + gs - 1) / gs;
    }
    return n;
}
// the prologue: encoders, edge build and the pp precompute of a dense conv layer 0, whichever of them this call needs
static int dyn_prologue(DynCall& dc) {
    pf_handle* h = dc.h; hipStream_t s = dc.s; const pf_config& c = h->cfg;
    // conv layer 0 on the row-group kernels: they encode the rows they read on the fly, only the edge build is launched
    // -- unless the previous denoising step's update launch has built the edges of these coordinates already
    dc.enc_fly = !dc.train && encoders_on_the_fly(h);
    // pocket sharing: copies of a pocket read one set of layer-0 pp messages (calls at one common t only)
    if (h->share_ok && h->share_check == 0) (void)share_now(h);                    // a claim about device rows: its verdict, whatever this call shares
    dc.share = dc.enc_fly && dc.t_scalar != nullptr && prune_layer(h) == 0 && share_now(h);
    if (h->share_check == 2)
        PF_FAIL(h, PF_ERR_ARG, "pf_set_pocket_groups: the claim made for this batch is false -- a graph differs from its representative in "
                               "coordinates or features (compared on the device); bind the batch again without the claim");
    if (h->edges_built && h->edges_share != dc.share) h->edges_built = false;    // built for the other mode: rebuild
    const BuildParams bp = build_params(h, dc.share);
    if (dc.enc_fly) { if (!h->edges_built) { ProfScope ps(h, pf_handle::K_BUILD, s); pfk_build_edges(&bp, s); build_done(h, dc.share); } }
    else if (h->prof_mask & 3u) {     // timing the two halves separately needs separate launches
        { ProfScope ps(h, pf_handle::K_ENCODE, s); pfk_encode(&dc.ep, s); }
        { ProfScope ps(h, pf_handle::K_BUILD, s); pfk_build_edges(&bp, s); }
    } else if (h->use_pre && h->Np > 0 && prune_layer(h) != 0) {      // layer 0 is dense: precompute P for its pp messages
        PreParams pp{};
        pp.Np = h->Np; pp.rec_nf = c.rec_nf; pp.nke = (c.rec_nf + 2) / 2;
        pp.prot_h0 = h->d_prot_h0; pp.t = dc.ep.t; pp.t_scalar = dc.ep.t_scalar; pp.gid = h->d_gid;
        pp.a_enc = h->d_w + h->pk.enc_a; pp.b_enc = h->d_w + h->pk.enc_bf; pp.ln_w = h->d_w + h->pk.enc_lw[0]; pp.ln_b = h->d_w + h->pk.enc_lb[0];
        pp.pre_w = h->h_gvp[h->msg_base(0, ET_PP)]; pp.pre_nks = 64 + c.rbf_dim / 2 + 9;
        pp.h_out = dc.ep.h_out; pp.pre_out = h->d_pre;
        pfk_encode_build_pre(&dc.ep, &bp, &pp, s); dc.pre_ready = true;
    } else pfk_encode_build(&dc.ep, &bp, s);
    return PF_OK;
}
// conv layer 0: static hoist of the pp messages (trajectory constants + per-timestep type table)
static void dyn_hoist_prepare(DynCall& dc) {
    pf_handle* h = dc.h; hipStream_t s = dc.s; const pf_config& c = h->cfg;
    dc.hoist = !dc.train && dc.enc_fly && l0_hoist_ok(h);
    // the n16 form serves the latency regime: batches whose pruned conv-layer launch has few items per compute unit
    dc.n16_batch = (long)(prune_layer(h) >= 0 ? h->n_edge_tiles_act : h->n_edge_tiles) * 32 <= h->pol.n16_rows_max && !h->pk.n16_msg.empty();
    dc.n16_l0 = dc.hoist && (h->pol.n16_mask & 2) && dc.n16_batch;      // layer 0 on the n16 kernels: no zs
    if (!dc.hoist) return;
    if (!dc.n16_l0) l0_ensure_static(h, s);
    if (dc.t_scalar) {
        l0_prepare_t(h, dc.t_scalar, 1, s);
        uint32_t bits; memcpy(&bits, dc.t_scalar, 4);
        dc.l0_ptab = h->d_ptab + (size_t)h->ptab_slot[bits] * L0_NTAB * c.rec_nf * PF_S;
    } else {
        L0HoistParams lp = l0_params(h);
        lp.nt = h->B; lp.t_dev = h->d_t; lp.ptab = h->d_ptab_pg;
        pfk_l0_hoist(&lp, 1, s);
        dc.l0_ptab = h->d_ptab_pg; dc.l0_gstride = L0_NTAB * c.rec_nf * PF_S;
    }
}
// n16 form (pf_n16.hip): 16-row items on four waves.  Conv layers >= 1 read h / v of the sources from memory; conv
// layer 0 needs the static hoist's type tables (protein sources) and encodes the centers on the fly
static void edge_n16_form(DynCall& dc, int l) {
    pf_handle* h = dc.h; EdgeParams& e = dc.e; const pf_config& c = h->cfg; const bool shared = dc.shared;
    for (int et = 0; et < 4; ++et) {
        e.n16[et] = h->d_w + (l > 0 ? h->pk.n16_msg[(size_t)l * 4 + et] : h->pk.n16_l0[et]);
        e.n16_stride[et] = (int)(l > 0 ? h->pk.n16_msg_stride : h->pk.n16_l0_stride[et]);
        e.ptab16_off[et] = et == ET_PP ? c.rec_nf * PF_S : (et == ET_PF ? 2 * c.rec_nf * PF_S : -1);
    }
    if (l == 0) { e.zs = nullptr; dc.rgp = 4; h->last_hoist = 16; }      // (ptab / ptype / l0_gid were set by edge_launch)
    if (l == 0 && dc.step != nullptr && h->run != RUN_NONE && !h->coords_custom) {
        // a sampling run: pp geometry from the original coordinates (the same bits in every step, with or without the rows
        // computed ahead; no race with the build that shifts xn under the speculative items)
        e.x0_static = h->d_prot_x0;
        // "pa" regions whose rows were computed ahead (k_n16_pa_spec) and still apply are skipped
        if (dc.spec_have && pa_ahead_ok(h, e, shared)) { e.pa_skip = h->d_pa_same; h->last_spec = 1; }
    }
    if (l == 0 && dc.cen_have && h->pk.n16_l0h[ET_FF] != 0) {              // ff / fp items start from the center hoist's tables (kind M0H)
        for (int et : {(int)ET_FF, (int)ET_FP}) { e.n16[et] = h->d_w + h->pk.n16_l0h[et]; e.n16_stride[et] = (int)h->pk.n16_l0h_stride[et]; }
        e.pcen = h->d_cen_p; e.pcen_nf = h->Nf; h->last_cen = true;
    }
    e.ngroups_sel = region_groups(h, shared, 0, e.nreg, 16);
    // conv layer 0, every graph with ff / pf / fp regions of one capacity: their items are mapped by arithmetic (k_n16_edge_u)
    int stride[3], cap[3], grp[3] = {0, 0, 0};
    bool uni = l == 0 && h->pol.fused_uni && !shared && e.reg == h->d_reg && e.nreg == 4 * h->B && h->B <= 64 && !e.pa_abs && !e.need &&
               uniform_regions(h, 3, stride, cap);
    for (int et = 0; et < 3 && uni; ++et) { grp[et] = (cap[et] + 15) / 16; uni = grp[et] > 0 && grp[et] < 8; }      // (three bits each)
    // k_n16_edge_u reaches pa_skip through the preloaded address of dyn_cnt, as an int offset (pfk_n16_edge): d_pa_same and d_dyn_cnt are
    // both carved from the workspace d_ws, so the offset is small -- a layout that breaks this takes the work-list form, here and there
    if (uni && e.pa_skip) { const long long off = (long long)(e.pa_skip - e.dyn_cnt); uni = off != 0 && off > -0x40000000LL && off < 0x40000000LL; }
    if (uni) {
        h->last_forms |= 1;
        for (int et = 0; et < 3; ++et) e.uni_base[et] = h->h_reg[(size_t)et * h->B];
        e.uni_s01 = stride[0] | (stride[1] << 16);
        e.uni_s2g = stride[2] | (grp[0] << 16) | (grp[1] << 19) | (grp[2] << 22) | ((h->B - 1) << 25);
        e.uni_pa_groups = region_groups(h, shared, 3 * h->B, 4 * h->B, 16);
    }
    dc.rg = 4;                               // 16 slots per partial-row group
    if (l == 0 && e.x0_static && pa_ahead_ok(h, e, shared)) {      // what k_n16_pa_spec needs of this launch (the regions, streams and tables of conv layer 0)
        e.cnt_snap = h->d_pa_cnt;                // (this launch leaves the kind-3 counts it consumed there: the speculative items' map)
        h->e0 = e; h->ep0 = dc.ep; h->e0_saved = true;
        h->e0_groups = region_groups(h, shared, 3 * h->B, 4 * h->B, 16);
    }
}
// the edge messages of conv layer l: form choice (LaunchPolicy) + launch
static void edge_launch(DynCall& dc, int l) {
    pf_handle* h = dc.h; hipStream_t s = dc.s; const pf_config& c = h->cfg; const bool train = dc.train;
    const bool last = dc.last = (l == c.n_convs - 1), pruned = dc.pruned = (l == prune_layer(h));
    EdgeParams& e = dc.e; int &rg = dc.rg, &rgp = dc.rgp;
    e = edge_params_base(h, l, last, pruned);
    e.h = train ? h->t_H[l] : h->d_h[dc.cur]; e.v = train ? h->t_V[l] : h->d_v[dc.cur];
    e.msg_s = train ? h->t_msg_s[l] : h->d_msg_s; e.msg_v = train ? h->t_msg_v[l] : h->d_msg_v;
    if (dc.fuse_l0node && l == 1) { e.msg_s = h->d_msg_s2; e.msg_v = h->d_msg_v2; }
    e.pre = (l == 0 && dc.pre_ready) ? h->d_pre : nullptr;
    if (train) { e.sv_z = h->t_sv_z[l]; e.sv_g = h->t_sv_g[l]; e.sv_v = h->t_sv_v[l]; e.sv_stride = (size_t)std::max<int64_t>(h->Ecap, 1); }
    // every edge of this launch lives in a dynamic region (each wave scans the region lengths: up to 1024 regions = 64 * RG_CPASS)
    const bool shared = dc.shared = dc.share && pruned && l == 0;       // pocket sharing: kind-3 regions = static ranges of the representatives
    if ((last || pruned) && h->rg_compact && (last ? 2 : 4) * h->B <= 1024) {
        e.reg = shared ? h->d_reg_share : h->d_reg; e.regB = h->B; e.nreg = (last ? 2 : 4) * h->B; e.pa_abs = shared ? 1 : 0;
        if (shared) { e.need = h->d_need; e.need_stamp = h->edges_stamp; }
        e.ngroups4 = region_groups(h, shared, 0, e.nreg, 4); e.ngroups8 = region_groups(h, shared, 0, e.nreg, 8);
    }
    // (bf16 leg: the message chains run on the 32-slot tile kernel, whose to_feats_out / gate products have a bf16 form)
    if (train && h->train_bf16) e.bf16 = 1;
    rg = train ? ((h->train_rg_edge && h->train_rg_node && !h->train_bf16) ? h->pol.rg_mode(e.ntiles) : 0)
               : h->pol.rg_mode(shared ? (int)((h->share_rows + 31) / 32) : e.ntiles);           // the node launch of this layer follows (partial-row grouping)
    // static hoist: the hoisted ("pa") items of a compact layer-0 launch run a two-block chain and may take 8 rows
    // per wave while the full-chain items (ff, pf, fp) take 4
    rgp = 0;
    if (dc.hoist && l == 0 && rg) {
        e.zs = h->d_zs; e.ptab = dc.l0_ptab; e.ptab_gstride = dc.l0_gstride; e.ptype = h->d_ptype; e.eorig = h->d_eorig; e.l0_gid = h->d_gid; e.l0c = h->d_l0c;
        rgp = rg;
        if (e.nreg > 0 && pruned) {
            // (a shared launch: most of the representatives' groups return at once, what runs scales with the batch like the dynamic regions
            // do -- the general threshold applies; measured at 4-5 pockets x 30 copies: 1.21 M sample-steps/s end to end at 4 rows per wave, 1.26 M at 8)
            // (one pocket x 128 copies: few shared rows, but 128 graphs' worth of ff / pf / fp items -- 8 rows per wave is 8 % ahead)
            rg = shared ? ((h->share_rows >= h->pol.rg2_rows_min || (long)e.ntiles * 32 >= h->pol.rg2_rows_min_hoist) ? 2 : 1)
                        : ((long)e.ntiles * 32 >= h->pol.rg2_rows_min_hoist ? 2 : 1);
            const int rgp_pol = shared ? rg : ((long)e.ntiles * 32 >= h->pol.rg2p_rows_min ? 2 : 1);
            if (h->pol.l0_rga) rg = h->pol.l0_rga;
            rgp = h->pol.l0_rgp ? h->pol.l0_rgp : std::max(rg, rgp_pol);
            if (rg == 2) rgp = 2;
            e.ngroups_sel = region_groups(h, shared, 0, 3 * h->B, 4 * rg) + region_groups(h, shared, 3 * h->B, e.nreg, 4 * rgp);     // (a pruned layer: nreg = 4 B)
        }
        h->last_hoist = 4 * rgp;
    }
    const bool n16e = !train && rg && dc.n16_batch && (l > 0 ? (h->pol.n16_mask & 1) != 0 : dc.n16_l0);
    if (n16e) edge_n16_form(dc, l);
    h->last_family.resize(c.n_convs);
    h->last_family[l] = rg ? 4 * rg : ((!train && e.ntiles <= ((last || pruned) ? std::max(h->pol.coop_edge_max, h->pol.coop2_edge_max) : std::max(h->pol.coop_edge_max, h->pol.coop2_dense_max))) ? 128 : 32);
    for (int et = 0; et < 4; ++et) { e.rgs[et] = h->d_w + h->pk.rgs_msg[(size_t)l * 4 + et]; e.rgs_stride = (int)h->pk.rgs_msg_stride; }
    const int esplit = (rg == 1 && e.ntiles * 8 <= h->pol.rg_split_max && !e.zs) ? 1 : 0;    // fewer groups than SIMDs: latency-bound
    const int pc = edge_prof_class(last, c.n_convs);
    if (n16e && dc.fuse_l0node && l == 1) {         // the fused launch: what conv layer 0's node update left in fz (fused_take_node) + its own fields
        FusedParams& fz = dc.fz;
        fz.chain[ET_FF] = h->d_w + h->pk.n16_fused[0]; fz.chain_stride[ET_FF] = (int)h->pk.n16_fused_stride[0];
        fz.chain[ET_PF] = h->d_w + h->pk.n16_fused[1]; fz.chain_stride[ET_PF] = (int)h->pk.n16_fused_stride[1];
        fz.upd_pharm = h->d_w + h->pk.n16_upd[(size_t)0 * 2 + 1]; fz.upd_pharm_stride = (int)h->pk.n16_upd_stride;
        fz.htab = dc.l0_ptab + (size_t)3 * c.rec_nf * PF_S; fz.htab_gstride = dc.l0_gstride; fz.ptype = h->d_ptype; fz.hcen = h->last_cen ? h->d_cen_h : nullptr;
        fz.h_out = h->d_h[dc.cur]; fz.v_out = h->d_v[dc.cur];          // (cur was flipped behind conv layer 0: its output side)
        fz.pharm_ptr = h->d_pharm_ptr; fz.Np = h->Np; fz.n_edge_items = e.ngroups_sel;
        fz.nff_cap = region_groups(h, shared, 0, std::min(h->B, e.nreg), 16); fz.npf_cap = region_groups(h, shared, h->B, e.nreg, 16);
        fz.xcd_split = ((h->pol.xcd_split & 1) && 2 * h->B <= 64 && h->max_nf <= 16) ? 1 : 0;
        // every graph with regions of one capacity (the same number of centers everywhere): the regions of an etype sit at a fixed
        // stride and the item map is arithmetic (k_n16_fused_u); PFDYN_FUSED_UNI=0: the work-list form
        int stride[2], cap[2];
        bool uni = fz.xcd_split && h->pol.fused_uni && e.reg == h->d_reg && e.nreg == 2 * h->B && uniform_regions(h, 2, stride, cap);
        for (int et = 0; et < 2 && uni; ++et) uni = cap[et] > 0 && (cap[et] + 15) / 16 < 256;      // (eight bits each)
        if (uni) {
            fz.uni_ff_base = h->h_reg[0]; fz.uni_pf_base = h->h_reg[(size_t)h->B];
            fz.uni_strides = stride[0] | (stride[1] << 16); fz.uni_groups = ((cap[0] + 15) / 16) | (((cap[1] + 15) / 16) << 8);
            h->last_forms |= 2 | (fz.rec ? 4 : 0);      // (k_n16_fused has no record path: its items chase their end points)
        }
        h->last_family[l] = 17;                      // pf_debug_kernel_family: 16-row items with conv layer 0's node update in front
        { ProfScope ps(h, pf_handle::K_EDGE_LAST, s); pfk_n16_fused(&e, &fz, &dc.ep, s); }
    }
    else if (n16e) {
        // PFDYN_PA_CHECK: the kept groups of the rows computed ahead must carry the serial of the launch that computed them (before this
        // launch overwrites the count snapshot the check compares with)
        if (l == 0 && e.pa_skip && h->d_pa_gstamp && h->d_pa_chk)
            pfk_pa_check(h->d_dyn_cnt, h->d_pa_cnt, e.reg, e.pa_skip, h->d_pa_gstamp, h->spec_serial, h->B, h->d_pa_chk, s);
        ProfScope ps(h, pc, s); pfk_n16_edge(&e, &dc.ep, l == 0, s);
    }
    else if (rg) { ProfScope ps(h, pc, s); pfk_rg_edge(&e, dc.enc_fly ? &dc.ep : nullptr, l == 0, rg, esplit, rgp, s); }
    // few tiles (last layer): 4 waves per tile to cut the serial latency; otherwise one wave per tile
    else if (e.ntiles <= h->pol.coop_edge_max && !train) { ProfScope ps(h, pc, s); pfk_edge_msg_coop(&e, l == 0, s); }
    else if (e.ntiles <= ((last || pruned) ? h->pol.coop2_edge_max : h->pol.coop2_dense_max) && !train) { ProfScope ps(h, pc, s); pfk_edge_msg_coop2(&e, l == 0, s); }
    else { ProfScope ps(h, pf_handle::K_EDGE, s); pfk_edge_msg(&e, l == 0, s); }
}
// the fused launch takes conv layer 0's node update: no node launch, the last layer's edge items (and its store items) compute these rows
static void fused_take_node(DynCall& dc, const NodeParams& n) {
    pf_handle* h = dc.h; FusedParams& fz = dc.fz;
    fz.in_start = n.in_start; fz.in_cnt = n.in_cnt; fz.N = n.N; fz.pp_slot = n.pp_slot;
    // (records describe the sources' in-edges as the update + build left them: the "pa" region as an atom's second segment)
    fz.rec = (h->rec_valid && h->d_rec && n.pp_slot == 2 && !dc.shared) ? h->d_rec : nullptr;
    fz.msg_s = n.msg_s; fz.msg_v = n.msg_v; fz.zero_row = n.zero_row; fz.grp = n.grp; fz.grp_pa = n.grp_pa;
    fz.gid = n.gid; fz.gnorm = n.gnorm; fz.B = n.B; fz.norm_mode = n.norm_mode; fz.norm_value = n.norm_value; fz.n_upd = n.n_upd;
    for (int nt = 0; nt < 2; ++nt) { fz.ln1_w[nt] = n.w[nt].ln1_w; fz.ln1_b[nt] = n.w[nt].ln1_b; fz.ln2_w[nt] = n.w[nt].ln2_w; fz.ln2_b[nt] = n.w[nt].ln2_b; }
}
static void node_save_levels(pf_handle* h, int l, NodeParams& n) {     // training forward: the update chains' levels stay for k_bwd_node
    n.sv_z = h->t_nsv_z[l]; n.sv_g = h->t_nsv_g[l]; n.sv_v = h->t_nsv_v[l]; n.sv_stride = (size_t)2 * h->N;
    h->t_node_saved[l] = 1;
}
// the tail launch: one workgroup per graph does the centers' node update, the head, the sampler update and the edge build.
// form 4: the row-group form (the fused node + head item, two per workgroup), 16: the n16 form
static void tail_launch(DynCall& dc, const NodeParams& n, int form) {
    pf_handle* h = dc.h; hipStream_t s = dc.s; const pf_config& c = h->cfg;
    const HeadParams hp = head_params(h, dc.eps_h, dc.eps_x); TailParams tp{};
    if (form == 16) {
        tp.in_start = n.in_start; tp.in_cnt = n.in_cnt; tp.N = n.N; tp.h_in = n.h_in; tp.v_in = n.v_in;
        tp.msg_s = n.msg_s; tp.msg_v = n.msg_v; tp.zero_row = n.zero_row; tp.grp = n.grp;
        tp.gid = n.gid; tp.gnorm = n.gnorm; tp.B = n.B; tp.norm_mode = n.norm_mode; tp.norm_value = n.norm_value;
        tp.ln1_w = n.w[1].ln1_w; tp.ln1_b = n.w[1].ln1_b; tp.ln2_w = n.w[1].ln2_w; tp.ln2_b = n.w[1].ln2_b;
        tp.n_upd = n.n_upd; tp.n_head = c.n_noise_gvps; tp.chain = h->d_w + h->pk.n16_tail; tp.chain_stride = (int)h->pk.n16_tail_stride;
        tp.pharm_nf = c.pharm_nf; tp.eps_h = dc.eps_h; tp.eps_x = dc.eps_x;
    }
    const bool sn = share_next(h);
    const BuildParams bpn = build_params(h, sn);
    { ProfScope ps(h, pf_handle::K_HEAD, s); if (form == 16) pfk_n16_tail(&tp, dc.step, &bpn, s); else pfk_rg_tail(&n, &hp, dc.step, &bpn, s); }
    build_done(h, sn);
    h->tail_done = true; h->last_tail = form; dc.head_done = true;
}
// center hoist for the NEXT call: its timestep from the announced plan (the entry behind this step's t); the tables
// serve a call that runs conv layer 0 on the n16 kernels with the type tables (as this one did); this step's
// features before the update must be in a snapshot (pf_sample_begin / the previous step left it).  NaN: no hoist
static float cen_hoist_plan(DynCall& dc) {
    pf_handle* h = dc.h;
    if (!(h->cen_hoist && dc.t_scalar && !h->t_plan.empty() && h->last_hoist == 16 && h->pk.l0c_off != 0 && h->pk.n16_l0h[ET_FF] != 0 &&
          h->snap_cur >= 0 && dc.step->h_snap_out != nullptr && h->d_xchg2 && dc.fuse_l0node)) return NAN;
    return planned_next_t(h, *dc.t_scalar, &h->plan_pos);
}
// ... and its workgroups' parameters
static void cen_hoist_params(DynCall& dc, float t_next, CenHoistParams& cp, HeadParams& hp) {
    pf_handle* h = dc.h; const StepParams* step = dc.step;
    cp.on = 1; cp.Nf = h->Nf; cp.nf = h->cfg.pharm_nf; cp.t_next = t_next; cp.pharm_h = h->d_snap[h->snap_cur]; cp.noise = step->noise;
    cp.a_ts = step->a_ts; cp.var = step->var; cp.sigma = step->sigma; cp.ep_zt = step->ep_zt; cp.ep_pred = step->ep_pred; cp.ep_feat = step->ep_feat;
    cp.enc_w = h->d_w + h->pk.enc_w[1]; cp.enc_b = h->d_w + h->pk.enc_b[1]; cp.enc_lw = h->d_w + h->pk.enc_lw[1]; cp.enc_lb = h->d_w + h->pk.enc_lb[1];
    cp.blk = h->d_w + h->pk.l0c_off; cp.cen_h = h->d_cen_h; cp.cen_p = h->d_cen_p; cp.xchg2 = hp.xchg2 = h->d_xchg2;
    h->cen_valid = true; h->cen_t = t_next; h->cen_wver = h->w_version;
}
// the NEXT call's "pa" messages, ahead of time, as workgroups of the merged launch (BuildParams::pa_same): conv layer 0's rows of this call have been
// consumed by the fused launch, the next timestep's type tables exist (or are made now).  Returns the number of speculative groups (0: none)
static int pa_ahead_plan(DynCall& dc, EdgeParams& es, EncodeParams& ees) {
    pf_handle* h = dc.h; const pf_config& c = h->cfg;
    if (!(h->e0_saved && h->pa_spec && !h->t_plan.empty() && dc.t_scalar && h->d_pa_stamp && !share_next(h))) return 0;
    float tn = planned_next_t(h, *dc.t_scalar, nullptr);
    if (tn != tn) return 0;
    l0_prepare_t(h, &tn, 1, dc.s);                  // (a no-op when the plan was announced)
    uint32_t bits; memcpy(&bits, &tn, 4);
    es = h->e0; es.pa_skip = nullptr; es.pcen = nullptr;
    es.ptab = h->d_ptab + (size_t)h->ptab_slot[bits] * L0_NTAB * c.rec_nf * PF_S;
    for (int et = 0; et < 4; ++et) { es.n16[et] = h->d_w + h->pk.n16_l0[et]; es.n16_stride[et] = (int)h->pk.n16_l0_stride[et]; }
    ees = h->ep0; ees.t_scalar = tn;
    h->spec_valid = true; h->spec_t = tn; h->spec_wver = h->w_version;
    es.pa_serial = h->spec_serial = ++h->pa_serial; es.pa_gstamp = h->d_pa_gstamp;
    return h->e0_groups;
}
// the merged last launch of a denoising step of a small batch: the step's update + build joins the node + head launch as
// workgroups of its own (k_rg_node_hs_build), with the work done ahead for the next call
static void merged_step_launch(DynCall& dc, const NodeParams& n, HeadParams& hp) {
    pf_handle* h = dc.h; hipStream_t s = dc.s; const pf_config& c = h->cfg;
    hp.xchg = h->d_xchg; hp.xchg_fault = h->xchg_fault;
    CenHoistParams cp{}; EdgeParams es{}; EncodeParams ees{};
    const float t_next = cen_hoist_plan(dc);
    const int spec_groups = pa_ahead_plan(dc, es, ees);
    if (t_next == t_next) cen_hoist_params(dc, t_next, cp, hp);
    const bool sn = share_next(h);
    BuildParams bpn = build_params(h, sn);
    // edge records for the next call's fused launch: radius ff edges, compact "pa" regions, the static hoist's element types
    const bool with_rec = h->d_rec && !sn && c.ff_k == 0 && bpn.act_ids && !bpn.pa_static && h->last_hoist == 16 && dc.fuse_l0node;
    if (with_rec) { bpn.rec = h->d_rec; bpn.ptype = h->d_ptype; }
    // PFDYN_PA_SPEC_SPLIT (test knob): no speculative slots in the merged launch; items w < k run just before it (the kind-3
    // counts before the build), w >= k just after it (the counts after the build).  "mid" / "step": k is half / a per-step
    // fraction of the non-empty groups, fixed by the launch in front (k_pa_spec)
    const bool split = spec_groups > 0 && h->pa_spec_split != 0;
    if (split) {
        const int frac = h->pa_spec_split == -1 ? 128 : (h->pa_spec_split == -2 ? (int)((((uint32_t)h->pa_serial * 2654435761u) >> 16) & 255) + 1 : 0);
        pfk_pa_spec(&es, &ees, spec_groups, 0, std::max(h->pa_spec_split, 0), frac, h->d_pa_cnt + h->B, s);
    }
    { ProfScope ps(h, pf_handle::K_HEAD, s); pfk_rg_node_hs_build(&n, &hp, dc.step, &bpn, h->d_xstat, h->pol.xchg_sleep, h->pol.hsb_avoid, h->xchg_poll_max, &cp, &es, &ees, split ? 0 : spec_groups, s); }
    if (split) pfk_pa_spec(&es, &ees, spec_groups, 1, 0, 0, h->d_pa_cnt + h->B, s);
    build_done(h, sn, with_rec);
    h->tail_done = true; h->last_tail = 2;
}
// the node update of conv layer l on the partial rows its edge launch left: form choice (LaunchPolicy) + launch
static void node_launch(DynCall& dc, int l) {
    pf_handle* h = dc.h; hipStream_t s = dc.s; const pf_config& c = h->cfg; const bool train = dc.train;
    NodeParams n = node_params_base(h, l, dc.last, dc.pruned);
    if (dc.shared) n.pp_slot = 3;
    n.msg_s = dc.e.msg_s; n.msg_v = dc.e.msg_v; n.h_in = dc.e.h; n.v_in = dc.e.v;
    n.h_out = train ? h->t_H[l + 1] : h->d_h[dc.cur ^ 1]; n.v_out = train ? h->t_V[l + 1] : h->d_v[dc.cur ^ 1];
    if (train) { n.drop_thr = h->t_common.drop_thr; n.drop_scale = h->t_common.drop_scale; n.seed = h->t_common.seed; n.layer = l; n.mask_override = h->t_common.mask_override; }
    n.grp = dc.rg ? 4 * dc.rg : 32; n.grp_pa = dc.rgp ? 4 * dc.rgp : n.grp;
    if (train) { h->t_grp.resize(c.n_convs); h->t_grp[l] = n.grp; h->t_node_saved.resize(c.n_convs); h->t_node_saved[l] = 0; }
    for (int nt = 0; nt < 2; ++nt) { n.rgs_upd[nt] = h->d_w + h->pk.rgs_upd[(size_t)l * 2 + nt]; n.rgs_stride[nt] = (int)h->pk.rgs_upd_stride[(size_t)l * 2 + nt]; }
    const EncodeParams* enc = dc.enc_fly ? &dc.ep : nullptr;
    if (dc.fuse_l0node && l == 0) fused_take_node(dc, n);
    else if (dc.rg) {
        const int rgn = (long)n.ntiles * 32 >= h->pol.rg2_rows_min_node ? 2 : 1;
        const bool fuse = dc.last && !train && h->fuse_head && h->n_head_tiles == n.ntiles;
        const int nsplit = (!train && rgn == 1 && n.ntiles * 8 <= (fuse ? h->pol.rg_split_max_head : h->pol.rg_split_max_node)) ? 1 : 0;
        const bool tail = fuse && dc.step != nullptr && l > 0 && (h->pol.n16_mask & 8) && h->B <= h->pol.tail_graphs_max && dc.enc_fly && step_build_fast_ok(h);
        if (tail) tail_launch(dc, n, (h->pol.tail_form == 16 && h->pk.n16_tail != 0) ? 16 : 4);
        else if (fuse) {
            // few two-wave items: confined to node_xcds XCDs when they fit one per compute unit there (32 CUs per XCD)
            if (nsplit && h->pol.node_xcds > 0 && n.ntiles * 8 <= 32 * h->pol.node_xcds) n.xcd_n = h->pol.node_xcds;
            if (nsplit && l > 0 && h->pol.node_static) { n.st_n0 = h->Np; n.st_n = h->Nf; }      // (the last layer's node tiles ARE the static tiling of the centers)
            HeadParams hp = head_params(h, dc.eps_h, dc.eps_x);
            // a denoising step of a small batch: the step's update + build joins this launch; timing the two separately needs the separate launches
            const bool hsb = n.st_n > 0 && dc.step != nullptr && h->pol.hs_build && dc.enc_fly && step_build_fast_ok(h) &&
                             h->B <= 256 && !(h->prof_mask & (1u << pf_handle::K_STEP)) && h->d_xchg && h->d_xstat;
            if (hsb) merged_step_launch(dc, n, hp);
            else { ProfScope ps(h, pf_handle::K_HEAD, s); pfk_rg_node(&n, &hp, enc, l == 0, rgn, nsplit, s); }
            dc.head_done = true;
        } else {
            if (train && h->train_node_save) node_save_levels(h, l, n);
            ProfScope ps(h, pf_handle::K_NODE_COOP, s); pfk_rg_node(&n, nullptr, enc, l == 0, rgn, nsplit, s);
        }
    }
    else if (dc.last && !train && h->fuse_head && n.ntiles <= h->pol.coop_node_max && h->n_head_tiles == n.ntiles) {
        // last layer (pharm tiles only) + noise head in one launch: the layer output stays in registers
        const HeadParams hp = head_params(h, dc.eps_h, dc.eps_x);
        { ProfScope ps(h, pf_handle::K_HEAD, s); pfk_node_head_coop(&n, &hp, l == 0, s); }
        dc.head_done = true;
    }
    else if (train && h->train_rg_node && h->pol.rg_mode(n.ntiles) > 0) {
        // training forward: the row-group node kernel (with the two GVPDropout sites) on the tile edge kernels' partial rows
        // (one per 32-slot tile and destination: grp = 32); the layer input comes from memory, as the backward kernels read it
        n.grp = 32; n.grp_pa = 32;
        if (h->train_node_save) node_save_levels(h, l, n);
        ProfScope ps(h, pf_handle::K_NODE_COOP, s); pfk_rg_node(&n, nullptr, nullptr, l == 0, h->pol.rg_mode(n.ntiles), 0, s);
    }
    else if (n.ntiles <= h->pol.coop_node_max && !train) { ProfScope ps(h, pf_handle::K_NODE_COOP, s); pfk_node_update_coop(&n, l == 0, s); }
    else { ProfScope ps(h, pf_handle::K_NODE, s); pfk_node_update(&n, l == 0, s); }
}
// the noise head as a launch of its own, when no node launch carried it
static void head_launch(DynCall& dc) {
    pf_handle* h = dc.h; hipStream_t s = dc.s; const pf_config& c = h->cfg; const bool train = dc.train;
    HeadParams hp = head_params(h, dc.eps_h, dc.eps_x);
    hp.h = train ? h->t_H[c.n_convs] : h->d_h[dc.cur]; hp.v = train ? h->t_V[c.n_convs] : h->d_v[dc.cur];
    if (train) h->t_head_saved = false;
    if (!dc.head_done && train && h->train_rg_head && !h->pk.rg_msg.empty() && h->Nf > 0) {
        // training forward: the head chain on the row-group code (4 rows per wave), which also leaves every level's pre-activations,
        // gate pre-activations and gated vectors for k_bwd_head (pharm rows are the contiguous rows [Np, Np + Nf))
        UnitParams up{};
        up.s_in = hp.h + (size_t)h->Np * PF_S; up.v_in = hp.v + (size_t)h->Np * 48; up.s_out = dc.eps_h; up.v_out = dc.eps_x;
        up.n = h->Nf; up.kind = 3; up.n_gvps = c.n_noise_gvps; up.pharm_nf = c.pharm_nf;
        up.stream = h->d_w + h->pk.rg_upd[(size_t)(c.n_convs - 1) * 2 + 1]; up.skip_gvps = c.n_update_gvps;
        up.sv_z = h->t_hsv_z; up.sv_g = h->t_hsv_g; up.sv_v = h->t_hsv_v; up.sv_stride = (size_t)h->Nf;
        { ProfScope ps(h, pf_handle::K_HEAD, s); pfk_rg_unit(&up, s); }
        h->t_head_saved = true; dc.head_done = true;
    }
    if (!dc.head_done) { ProfScope ps(h, pf_handle::K_HEAD, s); if (hp.ntiles <= h->pol.coop_node_max) pfk_noise_head_coop(&hp, s); else pfk_noise_head(&hp, s); }
}
// sequence one dynamics call on the handle's state (xn, pharm_h, d_t).  train: keep every layer's input and message rows (h->t_*), compute every
// tile (gradients need the full graph only where they are non-zero, but the first version of the backward pass walks the dense tile lists) and
// apply dropout in the node update.  step: this call is the dynamics call of a denoising step (pf_denoise_step) -- when the tail launch or the
// merged launch applies, the step's sampler update and edge build run behind the noise head in the same launch and h->tail_done tells the caller
static int run_dynamics(pf_handle* h, float* eps_h, float* eps_x, hipStream_t s, const float* t_scalar = nullptr, bool train = false, const StepParams* step = nullptr) {
    if (train ? h->train_wide : h->wide) return run_dynamics_wide(h, eps_h, eps_x, s, t_scalar, train);
    const pf_config& c = h->cfg;
    h->tail_done = false; h->last_tail = 0;
    DynCall dc{};
    dc.h = h; dc.s = s; dc.eps_h = eps_h; dc.eps_x = eps_x; dc.t_scalar = t_scalar; dc.train = train; dc.step = step;
    // center hoist: the previous denoising step left h_c and P_ff / P_fp of every center for THIS call's timestep
    dc.cen_have = !train && h->cen_valid && h->edges_built && t_scalar != nullptr && *t_scalar == h->cen_t && h->cen_wver == h->w_version;
    h->cen_valid = false; h->last_cen = false;
    // rows computed ahead for this call's "pa" regions (the speculative items of the previous step's merged launch)
    dc.spec_have = !train && h->spec_valid && h->edges_built && t_scalar != nullptr && *t_scalar == h->spec_t && h->spec_wver == h->w_version;
    h->spec_valid = false; h->last_spec = 0; h->last_forms = 0; h->e0_saved = false;
    if (!train) n16_refresh(h, s);
    dc.ep = encode_params(h, t_scalar, train ? h->t_H[0] : h->d_h[0]);
    if (const int rc = dyn_prologue(dc)) return rc;
    dyn_hoist_prepare(dc);
    h->last_hoist = 0;
    // fused launch (pf_n16.hip: k_n16_fused): with two conv layers, receptive-field pruning and kNN pf edges the rows conv layer 0's node update produces are
    // exactly the sources of the last layer's edges (+ the centers): every edge item of the last layer updates its own source rows first, and the node launch of conv layer 0 disappears
    dc.fuse_l0node = !train && dc.n16_batch && (long)h->n_edge_tiles_act * 32 <= h->pol.n16_fuse_rows_max && (h->pol.n16_mask & 4) && (h->pol.n16_mask & 1) && dc.hoist && c.n_convs == 2 && prune_layer(h) == 0 && c.pf_k > 0 &&
                     c.n_update_gvps >= 1 && h->rg_compact && 2 * h->B <= 1024 && h->d_msg_s2 != nullptr && h->pk.n16_fused[0] != 0;
    for (int l = 0; l < c.n_convs; ++l, dc.cur ^= 1) { edge_launch(dc, l); node_launch(dc, l); }
    head_launch(dc);
    h->edges_built = h->tail_done;          // whoever moves the coordinates next decides (pf_denoise_step rebuilds; the tail and merged launches have)
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return PF_OK;
}

// collects regions to clear and clears them with one launch (flush), eight at a time
struct ZeroBatch {
    ZeroList z{};
    hipStream_t s;
    explicit ZeroBatch(hipStream_t st) : s(st) {}
    void add(void* p, size_t nbytes) {
        if (!p || nbytes == 0) return;
        if (z.cnt == 8) flush();
        z.p[z.cnt] = p; z.nbytes[z.cnt] = nbytes; ++z.cnt;
    }
    void flush() { pfk_zero_multi(&z, s); z.cnt = 0; }
};

static int check_ready(pf_handle* h, bool need_batch) {
    if (!h) return PF_ERR_ARG;
    if (!h->committed) PF_FAIL(h, PF_ERR_STATE, "weights not committed (pf_commit_weights)");
    if (need_batch && !h->have_batch) PF_FAIL(h, PF_ERR_STATE, "no pocket batch set (pf_set_pocket_batch)");
    return PF_OK;
}

}  // namespace

// =================================================================================================
// class of every parameter tensor: the kernel that differentiates it.  The gradient path numbers its classes for n_convs <= 4:
// the list ends in front of the first tensor of a fifth conv layer (pf_commit_weights: n_tseg = -1, no gradient path)
static int tensor_classes(pf_handle* h, const FlatLayout& layout, std::vector<TensorSeg>& segs) {
    const pf_config& c = h->cfg;
    for (const auto& kv : layout) {
        const std::string& k = kv.first;
        TensorSeg sg{(int)kv.second.first, (int)(kv.second.first + kv.second.second), PFT_CLS_NONE, 0};
        if (kv.second.second == 0) sg.cls = PFT_CLS_NONE;
        else if (k.find("_encoder.") != std::string::npos) sg.cls = PFT_CLS_ENC;
        else if (k.find("noise_predictor.noise_predictor.") != std::string::npos) sg.cls = PFT_CLS_HEAD;
        else {
            int layer = -1;
            for (int l = 0; l < c.n_convs; ++l)
                if (k.compare(0, conv_prefix(l).size(), conv_prefix(l)) == 0) layer = l;
            if (layer < 0) PF_FAIL(h, PF_ERR_STATE, "internal: parameter %s has no gradient class", k.c_str());
            if (layer >= 4) break;
            sg.cls = PFT_CLS_NODE + layer;
            for (int et = 0; et < 4; ++et)
                if (k.find(std::string("edge_message_fns.") + kEtKey[et] + ".") != std::string::npos) sg.cls = PFT_CLS_MSG + layer * 4 + et;
        }
        segs.push_back(sg);
    }
    return PF_OK;
}

// flat range of the encoders' parameters: one contiguous run (the first tensors of the state dict)
static int encoder_range(pf_handle* h, const std::vector<TensorSeg>& segs, int& begin, int& n) {
    int lo = 0x7fffffff, hi = 0, tot = 0;
    for (const TensorSeg& sg : segs)
        if (sg.cls == PFT_CLS_ENC) { lo = std::min(lo, sg.begin); hi = std::max(hi, sg.end); tot += sg.end - sg.begin; }
    if (tot == 0) { lo = hi = 0; }
    if (hi - lo != tot) PF_FAIL(h, PF_ERR_STATE, "internal: the encoders' parameters are not contiguous in the flat layout");
    begin = lo; n = hi - lo;
    return PF_OK;
}

extern "C" {

const char* pf_version(void) { return "libpfdyn 0.1 (gfx950, fp32 MFMA)"; }

const char* pf_last_error(const pf_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int pf_create(const pf_config* cfg, pf_handle** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return PF_ERR_ARG; }
    *out = nullptr;
    auto bad = [&](const char* m) { g_create_error = m; return PF_ERR_ARG; };
    if (cfg->abi_version != PF_ABI_VERSION) return bad("abi_version mismatch");
    if (cfg->vector_size != 16 && cfg->vector_size != PFW_MAXV) return bad("vector_size must be 16 or 32");
    if (cfg->n_hidden_scalars < 64 || cfg->n_hidden_scalars > PFW_MAXS || cfg->n_hidden_scalars % 32)
        return bad("n_hidden_scalars must be a multiple of 32 in 64..256");
    if (cfg->rbf_dim != PF_R) return bad("rbf_dim must be 16");
    if (cfg->pharm_nf < 1 || cfg->pharm_nf > 16 || cfg->rec_nf < 1) return bad("pharm_nf must be in 1..16, rec_nf >= 1");
    if (cfg->n_convs < 1 || cfg->n_message_gvps < 1 || cfg->n_message_gvps > PF_MAX_GVPS || cfg->n_update_gvps < 1 ||
        cfg->n_update_gvps > PF_MAX_GVPS || cfg->n_noise_gvps < 1 || cfg->n_noise_gvps > PF_MAX_GVPS)
        return bad("layer counts out of range");
    if (cfg->ff_k < 0 || cfg->ff_k > PF_MAXK || cfg->pf_k < 0 || cfg->pf_k > PF_MAXK) return bad("ff_k / pf_k must be in 0..16");
    if (cfg->message_norm_mode < 0 || cfg->message_norm_mode > 2) return bad("bad message_norm_mode");
    if (cfg->message_norm_mode == PF_NORM_VALUE && !(cfg->message_norm_value > 0)) return bad("message_norm_value must be > 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        g_create_error = "no HIP device available (libpfdyn has no CPU fallback)";
        return PF_ERR_HIP;
    }
    pf_handle* h = new pf_handle();
    h->cfg = *cfg;
    h->init_tuning();
    // (128, 16) runs on the specialised kernels; every other pair, and (128, 16) under PFDYN_WIDE=1, on the width-generic family
    h->spec = cfg->n_hidden_scalars == PF_S && cfg->vector_size == PF_V;
    const char* wv = getenv("PFDYN_WIDE");
    h->wide = !h->spec || (wv && atoi(wv) != 0);
    if (h->wide) {              // the specialised path's hoists, speculation and merged launches do not apply
        h->l0_hoist = h->cen_hoist = h->pa_spec = false;
        h->pol.hs_build = 0; h->pol.n16_mask = 0;
    }
    *out = h;
    return PF_OK;
}

// (what the handle owns frees itself: pf_mem.h; the order: where pf_handle declares its streams and events)
void pf_destroy(pf_handle* h) {
    if (!h) return;
    delete h;
}

int pf_set_weight(pf_handle* h, const char* name, const float* host_data, int32_t ndim, const int64_t* shape) {
    if (!h || !name) return PF_ERR_ARG;
    int64_t n = 1;
    RawTensor t;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= shape[i]; }
    if (n == 0 || std::string(name) == "gamma.gamma") return PF_OK;     // dropout dummy_param / schedule table
    if (!host_data) PF_FAIL(h, PF_ERR_ARG, "null data for %s", name);
    t.data.assign(host_data, host_data + n);
    h->raw[name] = std::move(t);
    h->committed = false;
    return PF_OK;
}

int pf_commit_weights(pf_handle* h) {
    if (!h) return PF_ERR_ARG;
    const pf_config& c = h->cfg;
    // ---- on the host: everything that can fail without the device runs before the first old buffer is freed
    PackedModel pm;
    int rc = pack_model(c, h->raw, h->spec, h->wide, pm, h->err);
    if (rc) return rc;
    // gradient path: the parameters once more as one flat vector in state-dict order
    FlatLayout layout;
    ParamOffsets po;
    if ((rc = param_offsets(c, expected_tensors(c), layout, po, h->err)) != PF_OK) return rc;
    std::vector<float> flat;
    for (const auto& kv : layout) {
        const RawTensor& t = h->raw[kv.first];
        flat.insert(flat.end(), t.data.begin(), t.data.end());
    }
    std::vector<TensorSeg> segs;
    int enc_begin = 0, enc_n = 0;
    if ((rc = tensor_classes(h, layout, segs)) != PF_OK || (rc = encoder_range(h, segs, enc_begin, enc_n)) != PF_OK) return rc;
    // ---- the handle changes from here on.  A HIP call that fails leaves it uncommitted: some of its tables are then replaced, others not
    h->committed = false;
    h->flat_layout.swap(layout);
    h->po = std::move(po);
    h->enc_begin = enc_begin; h->enc_n = enc_n;
    h->pk = std::move(pm.lay);
    h->n_msg_tot = c.n_convs * 4 * c.n_message_gvps;
    h->n_upd_tot = c.n_convs * 2 * c.n_update_gvps;
    h->n_packed = pm.w.size();
    h->n_split_tab = pm.split_tab.size();
    PF_HIP(h, upload(h->d_w, pm.w));
    PF_HIP(h, upload(h->d_map, pm.map));
    PF_HIP(h, upload(h->d_split_tab, pm.split_tab));
    h->h_gvp.clear();
    for (const GvpOff& o : pm.gvp) {
        GvpW g;
        g.a_wh = h->d_w + o.wh; g.a_wu = h->d_w + o.wu; g.a_main = h->d_w + o.a_main; g.a_main_c = h->d_w + o.a_main_c; g.b_main = h->d_w + o.b_main;
        g.a_gate_c = h->d_w + o.a_gate_c; g.a_wh_c = h->d_w + o.wh_c; g.a_wu_c = h->d_w + o.wu_c;
        g.a_gate = h->d_w + o.a_gate; g.b_gate = h->d_w + o.b_gate;
        h->h_gvp.push_back(g);
    }
    PF_HIP(h, upload(h->d_gvp, h->h_gvp));
    h->nparams = flat.size();
    PF_HIP(h, upload(h->d_flat, flat));
    h->n_tseg = c.n_convs <= 4 ? (int)segs.size() : -1;
    PF_HIP(h, upload(h->d_tseg, segs));
    std::vector<GvpT> tab;              // where each GVP's tensors sit in the flat vector
    for_each_gvp(c, [&](const GvpSpec& g) {
        const int* o = &h->po.gvp[6 * tab.size()];
        GvpT t;
        t.o_Wh = o[0]; t.o_Wu = o[1]; t.o_Wm = o[2]; t.o_bm = o[3]; t.o_Wg = o[4]; t.o_bg = o[5];
        t.vi = g.vi; t.vo = g.vo; t.h = std::max(g.vi, g.vo); t.si = g.si; t.so = g.so; t.sig = 1;
        t.pk = (int)tab.size();
        tab.push_back(t);
    });
    tab.back().sig = 0;                 // the walk ends with the noise head's last GVP (pf_create: n_noise_gvps >= 1): no sigmoid on its vector gate
    h->n_gvpt = (int)tab.size();
    PF_HIP(h, upload(h->d_gvpt, tab));
    // per-handle allocations; what was derived from the old weights goes (ensure_wide_pack / the backward build theirs again on the new d_flat)
    h->d_wpack.release();
    h->wpack_version = ~0ull;
    h->d_wgvp.release(); h->d_wpk.release(); h->d_wpk_jobs.release();
    if (h->wide) {          // a handle of the family: its table points into d_w, and the gather map keeps that fresh
        std::vector<WideGvp> wtab;
        for_each_gvp(c, [&](const GvpSpec& g) {
            const size_t* o = &h->pk.wide_off[6 * wtab.size()];
            WideGvp w;
            w.wh = h->d_w + o[0]; w.wu = h->d_w + o[1]; w.wm = h->d_w + o[2]; w.bm = h->d_w + o[3]; w.wg = h->d_w + o[4]; w.bg = h->d_w + o[5];
            w.vi = g.vi; w.vo = g.vo; w.si = g.si; w.so = g.so;
            wtab.push_back(w);
        });
        PF_HIP(h, upload(h->d_wgvp, wtab));
    }
    PF_HIP(h, h->d_l0c.reserve(32 * sizeof(float), 32 * sizeof(float), Wait::none()));
    h->d_ptab.release();
    const size_t ptab_bytes = (size_t)L0_PTAB_SLOTS * L0_NTAB * c.rec_nf * PF_S * sizeof(float);
    if (h->spec) PF_HIP(h, h->d_ptab.reserve(ptab_bytes, ptab_bytes, Wait::none()));
    h->t_have_fwd = false;
    ++h->w_version;
    h->committed = true;
    return PF_OK;
}

// The bind's point of no return: the handle's fields take the plan's values, all in this one place.  The previous batch is gone
// (its training workspaces stay allocated and are carved again), and have_batch stays false until the bind has enqueued everything.
static void adopt_plan(pf_handle* h, const pfbind::BindPlan& p, const pfbind::BindInputs& in) {
    const int B = p.B;
    h->have_batch = false;
    free_ws(h, true);
    h->B = B; h->Np = p.Np; h->Nf = p.Nf; h->N = p.N; h->Epp = p.n_pp; h->Ecap = p.Ecap;
    h->h_prot_ptr.assign(in.prot_ptr, in.prot_ptr + B + 1);
    h->h_pharm_ptr.assign(in.pharm_ptr, in.pharm_ptr + B + 1);
    h->max_np = p.max_np; h->max_nf = p.max_nf;
    h->h_reg = p.h_reg; h->h_cap = p.h_cap;
    std::copy(p.et_tile0, p.et_tile0 + 5, h->et_tile0);
    std::copy(p.et_tile0_act, p.et_tile0_act + 5, h->et_tile0_act);
    h->n_edge_tiles = p.n_edge_tiles; h->n_node_tiles = p.n_node_tiles; h->n_head_tiles = p.n_head_tiles;
    h->n_edge_tiles_last = p.n_edge_tiles_last; h->n_node_tiles_last = p.n_node_tiles_last;
    h->n_edge_tiles_act = p.n_edge_tiles_act; h->n_node_tiles_act = p.n_node_tiles_act;
    h->share_ok = false; h->share_rows = 0;
    h->h_share_start.assign(B, 0); h->h_share_cnt.assign(B, 0);
}

// Every per-batch device pointer of the handle, from the plan's offsets: table section (tbase: the table buffer of this bind), zero
// section and scratch (base: the workspace); with them the flags that say what those buffers hold -- nothing yet.
static void set_batch_pointers(pf_handle* h, const pfbind::BindPlan& p, char* base, char* tbase) {
    const pf_config& c = h->cfg;
    const int Nf = p.Nf;
    auto at = [&](size_t o) { return base + o; };
    auto tat = [&](size_t o) { return tbase + o; };
    const pfbind::TableOff& ot = p.t;
    const pfbind::ZeroOff& oz = p.z;
    const pfbind::ScratchOff& os = p.s;
    h->d_prot_ptr = (int*)tat(ot.pptr); h->d_pharm_ptr = (int*)tat(ot.fptr); h->d_gid = (int*)tat(ot.gid); h->d_reg = (int*)tat(ot.reg);
    h->d_reg_act = (int*)tat(ot.regact); h->d_edge_tiles_act = (EdgeTile*)tat(ot.eta); h->d_node_tiles_act = (NodeTile*)tat(ot.nta);
    h->d_esrc = (int*)tat(ot.esrc); h->d_edst = (int*)tat(ot.edst); h->d_in_start = (int*)tat(ot.ins); h->d_in_cnt = (int*)tat(ot.inc);
    h->d_pp_cnt = (int*)tat(ot.ppc); h->d_edge_tiles = (EdgeTile*)tat(ot.et); h->d_node_tiles = (NodeTile*)tat(ot.nt);
    h->d_head_tiles = (NodeTile*)tat(ot.ht); h->d_pfq_cnt = p.pfq.empty() ? nullptr : (int*)tat(ot.pfq);
    h->d_reg_share = (int*)tat(ot.regs); h->d_pa_static = (int*)tat(ot.pas); h->d_rep_base = (int*)tat(ot.repb); h->d_need = (int*)at(oz.need);
    h->need_stamp = 0; h->edges_stamp = 0;
    h->d_dyn_cnt = (int*)at(oz.dyn); h->d_act_ids = (int*)at(oz.act); h->d_l0flag = (int*)at(oz.flag); h->d_gnorm = (float*)at(oz.gnorm);
    h->d_xn = (float4*)at(os.xn); h->d_prot_x0 = (float*)tat(ot.px0); h->d_prot_h0 = (float*)tat(ot.ph0); h->d_pharm_h = (float*)at(os.fh);
    h->d_t = (float*)at(os.t); h->d_h[0] = (float*)at(os.h0); h->d_h[1] = (float*)at(os.h1); h->d_v[0] = (float*)at(os.v0); h->d_v[1] = (float*)at(os.v1);
    h->d_msg_s2 = p.msg2 ? (float*)at(os.ms2) : nullptr; h->d_msg_v2 = p.msg2 ? (float*)at(os.mv2) : nullptr;
    h->d_msg_s = (float*)at(os.ms); h->d_msg_v = (float*)at(os.mv); h->d_eps_h = (float*)at(os.eh); h->d_eps_x = (float*)at(os.ex);
    h->d_com_init = (float*)at(os.c0); h->d_com_tmp = (float*)at(os.c1); h->d_pre = (float*)at(os.pre); h->d_eorig = (int*)at(os.eorig);
    h->d_ptype = (int*)at(os.ptype); h->d_zs = (float*)at(os.zs); h->d_ptab_pg = (float*)at(os.ptpg);
    h->d_rec = (h->pol.edge_rec && p.rec_slots > 0) ? (int4*)at(os.rec) : nullptr; h->rec_valid = false;
    h->d_xchg = (unsigned int*)at(os.xchg); h->d_lpart = (float*)at(oz.lpart);
    h->d_xchg2 = h->d_xchg + (size_t)std::max(Nf, 1) * PF_XCHG_STRIDE;
    h->d_cen_h = (float*)at(os.cenh); h->d_cen_p = (float*)at(os.cenp);
    h->d_snap[0] = (float*)at(os.snap); h->d_snap[1] = h->d_snap[0] + (size_t)std::max(Nf, 1) * c.pharm_nf + 4;
    h->cen_valid = false; h->snap_cur = -1;
    h->d_pa_stamp = (int*)at(oz.pastamp); h->d_pa_same = (int*)at(oz.pasame); h->spec_valid = false; h->e0_saved = false;
    h->d_pa_cnt = (int*)at(oz.pacnt); h->d_pa_gstamp = h->pa_check ? (int*)at(oz.pagst) : nullptr;
}

// ---- what arms the next begin (a seed: any begin; a pocket field and type guidance: a guided begin) and what a run leaves ----
// take: every public begin takes each arming off the handle on entry, before it can reject anything.  A bind drops every arming,
// rejected or not, and ends with no guided run on the batch (no source on, nothing for the pf_debug_last_* readers); a plain
// begin ends the guidance sources with their run
static bool take(bool& armed) { const bool was = armed; armed = false; return was; }
static void drop_armings(pf_handle* h) { h->seed_armed = h->field.armed = h->types.armed = h->pairs.armed = false; }
static void no_guided_run(pf_handle* h) { h->guide_have = h->field.on = h->field.have = h->types.on = h->types.have = h->pairs.on = h->pairs.have = false; }
static void end_guidance_sources(pf_handle* h) { h->field.on = h->types.on = h->pairs.on = false; }

// prot_x / prot_h come either as device pointers (copied on the stream) or as host pointers (staged with the tables).
// The arithmetic is pf_bind.cpp's (host only, checked on the CPU by tests/bind_check.cpp); this function owns the handle,
// the HIP resources and the enqueueing.
static int set_pocket_batch_impl(pf_handle* h, int32_t B, const int32_t* prot_ptr, const int32_t* pharm_ptr,
                                 const float* dev_prot_x, const float* dev_prot_h, const float* host_prot_x, const float* host_prot_h,
                                 int64_t n_pp, const int32_t* pp_src, const int32_t* pp_dst, pf_stream stream) {
    // ---- 1. the pocket-group claim (pf_set_pocket_groups) belongs to THIS bind: it is taken off the handle before anything
    // can fail, so that a rejected bind never leaves it behind for the next, unrelated batch
    pfbind::BindInputs in;
    if (h) in.rep.swap(h->pending_rep);
    if (h) drop_armings(h);                     // (so do a seed, a pocket field and type guidance: they are sized by and name the batch they came behind)
    if (h) h->ms_hist_valid = false;            // (and the multistep history: it belongs to a run on the batch before)
    int rc = check_ready(h, false);
    if (rc) return rc;
    const bool from_host = host_prot_x != nullptr;
    if (from_host ? !host_prot_h : (!dev_prot_x || !dev_prot_h)) PF_FAIL(h, PF_ERR_ARG, "pf_set_pocket_batch: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const pf_config& c = h->cfg;
    static const bool timing = getenv("PFDYN_TIMING") != nullptr;
    double tm[8] = {0}; int tmi = 0;
    auto now = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; };
    auto mark = [&] { if (timing && tmi < 8) tm[tmi++] = now(); };
    mark();
    // ---- 2. the plan: every argument check runs before the previous batch's state is touched -- a rejected bind leaves the
    // handle as it was
    in.cfg = c; in.B = B; in.prot_ptr = prot_ptr; in.pharm_ptr = pharm_ptr; in.n_pp = n_pp; in.pp_src = pp_src; in.pp_dst = pp_dst;
    in.host_rows = from_host; in.host_prot_x = host_prot_x; in.host_prot_h = host_prot_h;
    in.spec = h->spec; in.wide = h->wide; in.pa_check = h->pa_check; in.edge_rec = h->pol.edge_rec; in.n16_rows_max = h->pol.n16_rows_max;
#if defined(__x86_64__)
    static const bool avx2 = __builtin_cpu_supports("avx2") && getenv("PFDYN_NO_AVX2") == nullptr;
    in.allow_avx2 = avx2;
#endif
    pfbind::BindPlan p;
    pfbind::BindError berr;
    rc = pfbind::plan_batch(in, p, berr);
    if (rc) {
        if (berr.batch_lost) free_ws(h, true);         // (a batch too large for the edge slots' indices: the one rejection that drops the previous batch)
        h->err = berr.msg;
        return rc;
    }
    // ---- 3. the point of no return: from here on the handle describes the new batch (a failure below -- a false pocket-group
    // claim, a failing HIP call -- leaves it without a batch: loud, never the previous one's tables under the new sizes)
    adopt_plan(h, p, in);
    const int Np = p.Np, N = p.N;
    const int64_t Ecap = std::max<int64_t>(p.Ecap, 1);
    const size_t S = (size_t)c.n_hidden_scalars, V3 = (size_t)3 * c.vector_size;
    mark();      // 1: host tables built
    // ---- 4. the workspace, the table buffer of this bind and the staging buffer
    bool fresh = false;           // (launches of the previous batch may still read the old workspace: the device wait)
    PF_HIP(h, h->d_ws.reserve(p.ws_bytes + 4096, p.ws_bytes + p.ws_bytes / 8 + 4096, Wait::device(), &fresh));
    if (!h->d_xstat) {                                           // once per handle: the exchange's time-out counter and its pinned mirror
        PF_HIP(h, h->d_xstat.reserve(64, 64, Wait::none()));
        PF_HIP(h, hipMemset(h->d_xstat, 0, 64));
        PF_HIP(h, h->xstat_host.reserve(64, 64, Wait::none()));
        *h->xstat_host = 0; h->xstat_ack = 0;
    }
    pf_handle::TabSlot& tab = h->tab[h->tab_next];
    pf_handle::TabSlot& tab_other = h->tab[h->tab_next ^ 1];
    h->tab_next ^= 1;
    hipStream_t s_copy;
    PF_HIP(h, h->s_copy.get(&s_copy));
    bool tab_grew = false;        // (launches of two binds ago may still read the old buffer)
    PF_HIP(h, tab.buf.reserve(p.table_total + 4096, p.table_total + p.table_total / 8 + 4096, Wait::device(), &tab_grew));
    if (tab_grew) tab.guard.forget();
    // ---- 5. the pointers, from the plan's offsets
    char* const base = h->d_ws.as<char>();
    char* const tbase = tab.buf.as<char>();
    set_batch_pointers(h, p, base, tbase);
    if (h->pa_check && !h->d_pa_chk) {                           // once per handle: the check's counters
        PF_HIP(h, h->d_pa_chk.reserve(3 * sizeof(unsigned long long), 3 * sizeof(unsigned long long), Wait::none()));
        PF_HIP(h, hipMemset(h->d_pa_chk, 0, 3 * sizeof(unsigned long long)));
    }
    mark();      // 2: workspace ready
    // the tables are staged in pinned memory and uploaded with one asynchronous copy
    pf_handle::StageSlot& stage = h->stage[h->stage_next];
    h->stage_next ^= 1;
    PF_HIP(h, stage.ev.sync());                                  // the copy that last read this buffer (two binds ago) is done
    PF_HIP(h, stage.buf.reserve(p.table_bytes, p.table_bytes + p.table_bytes / 4 + 4096, Wait::none()));
    mark();      // 3: staging buffer ready
    // ---- 6. the table section, built in the staging buffer itself; a false pocket-group claim is rejected here
    char* const st = stage.buf.as<char>();
    pfbind::FillResult fr;
    rc = pfbind::fill_tables(p, in, st, fr, berr);
    if (rc) { h->err = berr.msg; return rc; }
    if (fr.share) {
        h->h_share_start.swap(fr.h_share_start); h->h_share_cnt.swap(fr.h_share_cnt);
        h->share_rows = fr.share_rows;
        h->share_ok = true;
    }
    mark();      // 4: staged
    // ---- 7. the upload: on the copy stream, once everything that read this table buffer (the bind before the previous one and
    // its steps) has finished; the caller's stream continues when it has arrived.  The guard of the OTHER buffer is recorded
    // now: what is enqueued on the caller's stream at this point is everything that reads it.
    PF_HIP(h, tab.guard.hold(s_copy));
    PF_HIP(h, tab_other.guard.record(s));
    PF_HIP(h, hipMemcpyAsync(tbase, st, p.table_bytes, hipMemcpyHostToDevice, s_copy));
    PF_HIP(h, stage.ev.record(s_copy));
    PF_HIP(h, tab.up.record(s_copy));
    PF_HIP(h, tab.up.hold(s));
    mark();      // 5: upload enqueued
    // ---- 8. the clears and the four launches.  Message rows: the node kernels read only rows the edge kernels of the same
    // layer wrote (the last slot of every aligned group a destination's segment touches) and the all-zero row Ecap, so a
    // reused workspace needs only that row cleared; a fresh allocation is cleared once in full
    {
        ZeroBatch zb(s);
        zb.add(base, p.zero_bytes);
        zb.add(h->d_v[0], (size_t)N * V3 * 4);
        if (fresh) {
            zb.add(h->d_msg_s, (size_t)(Ecap + 1) * S * 4);
            zb.add(h->d_msg_v, (size_t)(Ecap + 1) * V3 * 4);
        } else {
            zb.add(h->d_msg_s + (size_t)Ecap * S, S * 4);
            zb.add(h->d_msg_v + (size_t)Ecap * V3, V3 * 4);
        }
        if (h->d_msg_s2) {
            if (fresh) {
                zb.add(h->d_msg_s2, (size_t)(Ecap + 1) * PF_S * 4);
                zb.add(h->d_msg_v2, (size_t)(Ecap + 1) * 48 * 4);
            } else {
                zb.add(h->d_msg_s2 + (size_t)Ecap * PF_S, PF_S * 4);
                zb.add(h->d_msg_v2 + (size_t)Ecap * 48, 48 * 4);
            }
        }
        zb.flush();
    }
    h->zero_row = (int)Ecap;
    if (!from_host) {
        pfk_copy2(dev_prot_x, h->d_prot_x0, (size_t)Np * 3, dev_prot_h, h->d_prot_h0, (size_t)Np * c.rec_nf, s);
    }
    h->share_check = 1;
    if (!from_host && h->share_ok) {             // the claim's rows are on the device only: compared there, verdict read back lazily
        pfk_verify_copies(h->d_prot_x0, h->d_prot_h0, h->d_gid, h->d_prot_ptr, h->d_rep_base, Np, c.rec_nf, h->d_l0flag + 1, s);
        h->share_check = 0;
    }
    pfk_load_coords(h->d_prot_x0, h->d_xn, Np, h->d_gid, nullptr, 0.f, s);
    {
        L0HoistParams lp{};
        lp.prot_h0 = h->d_prot_h0; lp.Np = Np; lp.rec_nf = c.rec_nf; lp.ptype = h->d_ptype; lp.flag = h->d_l0flag;
        lp.zs = reinterpret_cast<float*>(h->d_eorig); lp.Epp = (int)Ecap;      // static slot of every edge slot: the identity
        pfk_l0_hoist(&lp, 2, s);
    }
    // ---- 9. the read-back: the one-hot verdict of k_l0_types comes back through pinned memory; nobody waits for it here
    // (l0_resolve_onehot)
    PF_HIP(h, h->l0flag_host.reserve(64, 64, Wait::none()));
    PF_HIP(h, h->l0flag_ev.sync());                              // the previous bind's read-back (long done) before its target is reused
    h->l0flag_host[0] = 1; h->l0flag_host[1] = 1;
    PF_HIP(h, hipMemcpyAsync(h->l0flag_host, h->d_l0flag, 8, hipMemcpyDeviceToHost, s));
    PF_HIP(h, h->l0flag_ev.record(s));
    mark();      // 6: everything enqueued
    if (timing) fprintf(stderr, "[pf_set_pocket_batch] B=%d checks+tables %.2f ws %.2f stage-wait %.2f index arrays (in staging) %.2f upload %.2f launches+waits %.2f ms (fresh %d, %zu MB)\n",
                        B, tm[1] - tm[0], tm[2] - tm[1], tm[3] - tm[2], tm[4] - tm[3], tm[5] - tm[4], tm[6] - tm[5], (int)fresh, p.ws_bytes >> 20);
    // ---- 10. the per-batch flags
    h->l0_state = 0; h->l0_onehot = false;
    if (fr.host_onehot >= 0) { h->l0_state = fr.host_onehot ? 1 : 2; h->l0_onehot = fr.host_onehot == 1; }
    h->zs_version = 0; h->zs_batch_coords = false; h->coords_custom = false;
    h->have_batch = true;
    h->run = RUN_NONE; no_guided_run(h);
    h->edges_built = false; h->rec_valid = false;
    return PF_OK;
}

int pf_set_pocket_batch(pf_handle* h, int32_t B, const int32_t* prot_ptr, const int32_t* pharm_ptr,
                        const float* dev_prot_x, const float* dev_prot_h, int64_t n_pp, const int32_t* pp_src,
                        const int32_t* pp_dst, pf_stream stream) {
    if (h && (!dev_prot_x || !dev_prot_h)) {
        h->pending_rep.clear();                  // a pocket-group claim never outlives the bind it was made for, rejected or not
        drop_armings(h);
        PF_FAIL(h, PF_ERR_ARG, "pf_set_pocket_batch: bad argument");
    }
    return set_pocket_batch_impl(h, B, prot_ptr, pharm_ptr, dev_prot_x, dev_prot_h, nullptr, nullptr, n_pp, pp_src, pp_dst, stream);
}

int pf_set_pocket_batch_host(pf_handle* h, int32_t B, const int32_t* prot_ptr, const int32_t* pharm_ptr,
                             const float* host_prot_x, const float* host_prot_h, int64_t n_pp, const int32_t* pp_src,
                             const int32_t* pp_dst, pf_stream stream) {
    if (h && (!host_prot_x || !host_prot_h)) {
        h->pending_rep.clear();
        drop_armings(h);
        PF_FAIL(h, PF_ERR_ARG, "pf_set_pocket_batch_host: bad argument");
    }
    return set_pocket_batch_impl(h, B, prot_ptr, pharm_ptr, nullptr, nullptr, host_prot_x, host_prot_h, n_pp, pp_src, pp_dst, stream);
}

int pf_set_pocket_groups(pf_handle* h, int32_t B, const int32_t* host_rep) {
    if (!h) return PF_ERR_ARG;
    if (B < 0 || (B > 0 && !host_rep)) PF_FAIL(h, PF_ERR_ARG, "pf_set_pocket_groups: bad argument");
    h->pending_rep.assign(host_rep, host_rep + B);
    return PF_OK;
}

int pf_declare_onehot_features(pf_handle* h, int32_t is_onehot) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    h->l0_state = is_onehot ? 1 : 2;
    h->l0_onehot = is_onehot != 0 && h->Np > 0;
    return PF_OK;
}

int64_t pf_build_pp_edges(pf_handle* h, int32_t B, const int32_t* prot_ptr, const float* dev_prot_x, int32_t max_nb,
                          int32_t* host_src, int32_t* host_dst, int64_t capacity, pf_stream stream) {
    if (!h || B < 1 || !prot_ptr || !dev_prot_x) return PF_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int Np = prot_ptr[B];
    DevArr<float4> xn; DevArr<int> dptr, ddeg, doff, dsrc, ddst;     // (every return frees them)
    std::vector<int> deg(std::max(Np, 1)), off(std::max(Np, 1) + 1, 0);
    int64_t total = 0;
    auto alloc = [](auto& b, size_t bytes) { return b.reserve(bytes, bytes, Wait::none()); };
    PF_HIP(h, alloc(xn, (size_t)std::max(Np, 1) * 16));
    PF_HIP(h, alloc(dptr, (size_t)(B + 1) * 4));
    PF_HIP(h, alloc(ddeg, (size_t)std::max(Np, 1) * 4));
    PF_HIP(h, alloc(doff, (size_t)std::max(Np, 1) * 4));
    PF_HIP(h, hipMemcpy(dptr, prot_ptr, (size_t)(B + 1) * 4, hipMemcpyHostToDevice));
    pfk_load_coords(dev_prot_x, xn, Np, nullptr, nullptr, 0.f, s);
    const float r2 = h->cfg.cutoff_pp * h->cfg.cutoff_pp;
    pfk_pp_radius(xn, dptr, B, r2, max_nb, ddeg, nullptr, nullptr, nullptr, 0, s);
    PF_HIP(h, hipStreamSynchronize(s));
    PF_HIP(h, hipMemcpy(deg.data(), ddeg, (size_t)Np * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < Np; ++i) { off[i] = (int)total; total += deg[i]; }
    if (host_src && host_dst) {
        if (capacity < total) PF_FAIL(h, PF_ERR_ARG, "pf_build_pp_edges: capacity too small");
        if (total > 0) {
            PF_HIP(h, alloc(dsrc, (size_t)total * 4));
            PF_HIP(h, alloc(ddst, (size_t)total * 4));
            PF_HIP(h, hipMemcpy(doff, off.data(), (size_t)Np * 4, hipMemcpyHostToDevice));
            pfk_pp_radius(xn, dptr, B, r2, max_nb, ddeg, doff, dsrc, ddst, 1, s);
            PF_HIP(h, hipStreamSynchronize(s));
            PF_HIP(h, hipMemcpy(host_src, dsrc, (size_t)total * 4, hipMemcpyDeviceToHost));
            PF_HIP(h, hipMemcpy(host_dst, ddst, (size_t)total * 4, hipMemcpyDeviceToHost));
        }
    }
    return total;
}

static int load_state(pf_handle* h, const float* dev_prot_x, const float* dev_pharm_x, const float* dev_pharm_h, hipStream_t s) {
    h->edges_built = false; h->rec_valid = false;
    if (dev_prot_x) { pfk_load_coords(dev_prot_x, h->d_xn, h->Np, h->d_gid, nullptr, 0.f, s); h->coords_custom = true; }
    if (dev_pharm_x) pfk_load_coords(dev_pharm_x, h->d_xn + h->Np, h->Nf, h->d_gid, nullptr, 0.f, s);
    if (dev_pharm_h) pfk_copy(dev_pharm_h, h->d_pharm_h, (size_t)h->Nf * h->cfg.pharm_nf, s);
    return PF_OK;
}

int pf_dynamics_forward(pf_handle* h, const float* dev_prot_x, const float* dev_pharm_x, const float* dev_pharm_h,
                        const float* dev_t, float* dev_eps_h, float* dev_eps_x, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!dev_pharm_x || !dev_pharm_h || !dev_t || !dev_eps_h || !dev_eps_x) PF_FAIL(h, PF_ERR_ARG, "pf_dynamics_forward: null argument");
    hipStream_t s = (hipStream_t)stream;
    load_state(h, dev_prot_x, dev_pharm_x, dev_pharm_h, s);
    pfk_copy(dev_t, h->d_t, (size_t)h->B, s);
    return run_dynamics(h, dev_eps_h, dev_eps_x, s);
}

static int seed_move(pf_handle* h, const float* dev_noise0, hipStream_t s);
// A pocket field, type guidance and pair guidance arm the next GUIDED begin; the begin of any other run kind drops them and says so.  (A seed
// arms the next begin of any kind, which hands `seeded` down to the begin it is built on)
static int refuse_field(pf_handle* h, const char* who) {
    const bool fielded = h && take(h->field.armed), typed = h && take(h->types.armed), paired = h && take(h->pairs.armed);
    if (fielded) PF_FAIL(h, PF_ERR_STATE, "%s while a pocket field is armed (pf_guide_field_next arms pf_sample_begin_guided / pf_sample_guided "
                                          "only): the arming is dropped", who);
    if (typed) PF_FAIL(h, PF_ERR_STATE, "%s while type guidance is armed (pf_guide_types_next arms pf_sample_begin_guided / pf_sample_guided "
                                        "only): the arming is dropped", who);
    if (paired) PF_FAIL(h, PF_ERR_STATE, "%s while pair guidance is armed (pf_guide_pairs_next arms pf_sample_begin_guided / pf_sample_guided "
                                         "only): the arming is dropped", who);
    return PF_OK;
}

static int begin_plain(pf_handle* h, const float* dev_init_pharm_com, const float* dev_noise0, bool seeded, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!dev_noise0) PF_FAIL(h, PF_ERR_ARG, "pf_sample_begin: null noise");
    {                                       // a caller that never asked pf_sample_status still learns of an invalid run here
        int32_t n = 0;
        rc = pf_sample_status(h, &n);
        if (rc) return rc;
    }
    hipStream_t s = (hipStream_t)stream;
    // every run starts from armed exchange words, whatever the previous run on the handle left in them (a timed-out row is not
    // re-armed by its consumer, pf_stepbuild.h); stream-ordered like everything else of the run
    if (h->d_xchg) PF_HIP(h, hipMemsetAsync(h->d_xchg, 0xff, (size_t)2 * std::max(h->Nf, 1) * PF_XCHG_STRIDE * sizeof(unsigned int), s));
    // init_prot_com = mean of the ORIGINAL protein coordinates (pharmacodiff.py:442)
    pfk_load_coords(h->d_prot_x0, h->d_xn, h->Np, h->d_gid, nullptr, 0.f, s);
    pfk_segment_mean(h->d_xn, h->d_prot_ptr, 0, h->B, h->d_com_init, s);
    const float* shift = dev_init_pharm_com ? dev_init_pharm_com : h->d_com_init;      // :448-452
    pfk_load_coords(h->d_prot_x0, h->d_xn, h->Np, h->d_gid, shift, -1.f, s);
    if (!seeded) pfk_load_noise0(dev_noise0, h->d_xn + h->Np, h->d_pharm_h, h->Nf, h->cfg.pharm_nf, s);  // :455-456
    h->cen_valid = false; h->snap_cur = -1;
    h->spec_valid = false; h->step_id += 2;      // (a gap: no stamp of the run before reads as "the previous step")
    if (!seeded && h->cen_hoist && h->d_snap[0] && h->pk.l0c_off != 0) {      // center hoist: the features as they are, for the first step's hoist workgroups
        pfk_copy(h->d_pharm_h, h->d_snap[0], (size_t)h->Nf * h->cfg.pharm_nf, s);
        h->snap_cur = 0;
    }
    h->coords_custom = false;               // a rigid translate of the batch's own coordinates from here on
    h->run = RUN_PLAIN;
    end_guidance_sources(h);
    h->ms_hist_valid = false;               // a run begins without a previous output
    h->edges_built = false; h->rec_valid = false;
    // a seeded begin: the state is the noised seed, made by a move of the step end (which also writes the snapshot, after the move)
    return seeded ? seed_move(h, dev_noise0, s) : PF_OK;
}
int pf_sample_begin(pf_handle* h, const float* dev_init_pharm_com, const float* dev_noise0, pf_stream stream) {
    const bool seeded = h && take(h->seed_armed);
    if (const int rc = refuse_field(h, "pf_sample_begin")) return rc;
    return begin_plain(h, dev_init_pharm_com, dev_noise0, seeded, stream);
}

// ---- the sampler's run state: one guard for the entry points that need a run in progress ----
// One row per run kind: its name, the call that begins it, and what it tells a caller that belongs to a lesser kind -- the step
// to use instead, and what becomes of a resampling jump.  The kinds are ordered by what they add: a guided run is a pinned run
// is a plain run, so a caller's kind below the run's is "inside", above it "outside".
static const struct { const char *name, *begin, *step, *jump; } RUN_ROWS[] = {
    {nullptr, nullptr, nullptr, nullptr},
    {"plain", "pf_sample_begin", "use pf_denoise_step", nullptr},
    {"pinned", "pf_sample_begin_pinned", "use pf_denoise_step_pinned", "use pf_renoise_step"},
    {"guided", "pf_sample_begin_guided", "use pf_denoise_step_guided", "guidance with resampling jumps is not supported"},
};
// who: the caller; needs: the run kind it belongs to (RUN_NONE: any run in progress will do); jump: the caller is a resampling jump
static int run_guard(pf_handle* h, const char* who, RunKind needs, bool jump = false) {
    if (needs == RUN_NONE ? h->run != RUN_NONE : h->run == needs) return PF_OK;
    if (needs == RUN_NONE) PF_FAIL(h, PF_ERR_STATE, "no sampling run in progress");
    if (h->run > needs) PF_FAIL(h, PF_ERR_STATE, "%s inside a %s run (%s): %s", who, RUN_ROWS[h->run].name, RUN_ROWS[h->run].begin,
                                jump ? RUN_ROWS[h->run].jump : RUN_ROWS[h->run].step);
    if (needs == RUN_PLAIN) PF_FAIL(h, PF_ERR_STATE, "%s before pf_sample_begin", who);
    PF_FAIL(h, PF_ERR_STATE, "%s outside a %s run (%s)", who, RUN_ROWS[needs].name, RUN_ROWS[needs].begin);
}

// ---- one builder per parameter struct of a step ----
// what every move reads: the batch, the state and the step's noise (a re-noise move reads nothing else)
static StepParams step_params_base(const pf_handle* h, const float* dev_noise) {
    StepParams sp{};
    sp.B = h->B; sp.Np_tot = h->Np; sp.prot_ptr = h->d_prot_ptr; sp.pharm_ptr = h->d_pharm_ptr;
    sp.xn = h->d_xn; sp.pharm_h = h->d_pharm_h; sp.noise = dev_noise; sp.nf = h->cfg.pharm_nf;
    return sp;
}
// the p(z_s | z_t) update's parameters of one denoising step (h_snap_out is the caller's)
static StepParams step_params(const pf_handle* h, const pf_step_coef* coef, const float* dev_noise, int32_t ep_coord, int32_t ep_feat) {
    StepParams sp = step_params_base(h, dev_noise);
    sp.eps_h = h->d_eps_h; sp.eps_x = h->d_eps_x;
    sp.a_ts = coef->alpha_t_given_s; sp.var = coef->var_terms; sp.sigma = coef->sigma;
    sp.ep_zt = coef->ep_zt; sp.ep_pred = coef->ep_pred; sp.ep_coord = ep_coord; sp.ep_feat = ep_feat;
    return sp;
}
// the run's pin arrays at this step's noise level (pinned and guided steps)
static PinParams pin_params(const pf_handle* h, const pf_pin_coef* pin) {
    PinParams q{};
    q.flags = h->d_pin_flags; q.pin_x = h->d_pin_x; q.pin_h = h->d_pin_h; q.com_init = h->d_com_init;
    q.alpha_s = pin->alpha_s; q.sigma_s = pin->sigma_s; q.feat_norm = h->pin_feat_norm;
    return q;
}

// ---- one step end ----
// The move a step's own last launch makes.  build_form: the move has an "update + edge build in one launch" form (the guided
// move has none: the width-generic training forward in front of it builds its own edges on every call)
struct StepMove {
    StepMoveArgs args{};                    // the tag and what the move's kernel reads (pf_device.h)
    bool build_form = true;
    int snap_next = -1;                     // PLAIN, SEED: the snapshot sp.h_snap_out is (center hoist)
};
// What every op calls after its dynamics call (if it has one): the move, unless the dynamics call's tail or merged launch made
// it already; what the move leaves of the edges; what survives of the work done ahead (snapshot, center hoist, speculative rows)
static int step_end(pf_handle* h, const StepParams& sp, const StepMove& mv, hipStream_t s) {
    const StepMoveArgs::Kind kind = mv.args.kind;
    const bool plain = kind == StepMoveArgs::PLAIN;
    const bool moved = plain && h->tail_done;       // (only a plain step hands its StepParams to run_dynamics)
    if (!moved) {
        // the move + the edges of the next dynamics call in one launch, or the move alone
        const bool build = mv.build_form && encoders_on_the_fly(h), share = build && share_next(h);
        const BuildParams bp = build ? build_params(h, share) : BuildParams{};
        {
            ProfScope ps(h, pf_handle::K_STEP, s);
            if (plain && build && step_build_fast_ok(h)) pfk_step_build_fast(&sp, &bp, s);
            else pfk_step_move(&sp, &mv.args, build ? &bp : nullptr, s);
        }
        if (build) build_done(h, share);
        else h->rec_valid = false;                  // the centers moved: the next dynamics call builds
        h->edges_built = build;
    }
    // a re-noise move has no dynamics call in front of it that would have reset these
    if (!plain) { h->tail_done = false; h->last_tail = 0; }
    // the multistep history holds the outputs of the step in front of this move only if that move wrote it
    h->ms_hist_valid = kind == StepMoveArgs::MS;
    // the work done ahead is for the state the merged launch of a plain step left: every other move invalidates it.  The seed
    // move opens a run: nothing is ahead of it, and the snapshot it wrote holds the features as they are now
    const bool ahead = plain && h->tail_done && h->last_tail == 2;
    h->snap_cur = ((ahead || kind == StepMoveArgs::SEED) && sp.h_snap_out) ? mv.snap_next : -1;
    if (h->snap_cur < 0) h->cen_valid = false;
    if (!ahead) h->spec_valid = false;
    const hipError_t e = moved ? hipSuccess : hipGetLastError();     // (run_dynamics has checked the tail and merged launches)
    if (e != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return PF_OK;
}

int pf_denoise_step(pf_handle* h, const pf_step_coef* coef, const float* dev_noise, int32_t ep_coord, int32_t ep_feat,
                    pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!coef || !dev_noise) PF_FAIL(h, PF_ERR_ARG, "pf_denoise_step: null argument");
    if ((rc = run_guard(h, __func__, RUN_PLAIN)) != PF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    StepParams sp = step_params(h, coef, dev_noise, ep_coord, ep_feat);
    // center hoist: the updated features also go to the snapshot the NEXT step's hoist workgroups read (they must not race with that
    // step's update of pharm_h); only the paths through pf_stepbuild.h write it
    ++h->step_id;
    const int snap_next = h->snap_cur < 0 ? 0 : (h->snap_cur ^ 1);
    sp.h_snap_out = (h->cen_hoist && h->d_snap[0] && h->pk.l0c_off != 0) ? h->d_snap[snap_next] : nullptr;
    rc = run_dynamics(h, h->d_eps_h, h->d_eps_x, s, &coef->t, false, &sp);      // every graph of the batch is at the same t
    if (rc) return rc;
    StepMove mv;
    mv.args.kind = StepMoveArgs::PLAIN; mv.snap_next = snap_next;
    return step_end(h, sp, mv, s);
}

// The seeded begin's move (pf_sample_seed_next): every center becomes the seed noised to the run's first level with the initial
// draw; the snapshot the first plain step's hoist workgroups read is written by the move itself
static int seed_move(pf_handle* h, const float* dev_noise0, hipStream_t s) {
    StepParams sp = step_params_base(h, dev_noise0);
    sp.h_snap_out = (h->cen_hoist && h->d_snap[0] && h->pk.l0c_off != 0) ? h->d_snap[0] : nullptr;
    StepMove mv;
    mv.args.kind = StepMoveArgs::SEED; mv.snap_next = 0;
    SeedParams& q = mv.args.seed;
    q.seed_x = h->d_seed_x; q.seed_h = h->d_seed_h; q.com_init = h->d_com_init;
    q.alpha_a = h->seed_alpha; q.sigma_a = h->seed_sigma; q.feat_norm = h->seed_feat_norm;
    return step_end(h, sp, mv, s);
}

// A run's device scratch (d_pin, d_guide, d_seed, a staged block's device buffer) is kept while it fits.  Launches of an earlier run
// on the caller's stream may still read it, so replacing it waits for that STREAM (Wait::on(s)) -- not for the device as a bind's
// buffers do: several lanes sample on one device at once

// Pinned centers: pf_sample_begin, then the handle's own copy of the caller's pin arrays (stream-ordered; the caller may free its
// arrays once the stream has passed this call).  The run is pinned until the next pf_sample_begin / _pinned or bind
static int begin_pinned(pf_handle* h, const float* dev_init_pharm_com, const float* dev_noise0, const int32_t* dev_pin_flags,
                        const float* dev_pin_x, const float* dev_pin_h, float feat_norm_constant, bool seeded, pf_stream stream) {
    if (h && (!dev_pin_flags || !dev_pin_x || !dev_pin_h)) PF_FAIL(h, PF_ERR_ARG, "pf_sample_begin_pinned: null pin array");
    if (h && !(feat_norm_constant > 0.f)) PF_FAIL(h, PF_ERR_ARG, "pf_sample_begin_pinned: feat_norm_constant must be positive");
    int rc = begin_plain(h, dev_init_pharm_com, dev_noise0, seeded, stream);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t nf = (size_t)std::max(h->Nf, 1), nh = (size_t)h->cfg.pharm_nf;
    const size_t bytes = nf * 4 * (1 + 3 + nh);
    PF_HIP(h, h->d_pin.reserve(bytes, bytes, Wait::on(s)));
    h->d_pin_flags = h->d_pin.as<int>(); h->d_pin_x = h->d_pin.as<float>() + nf; h->d_pin_h = h->d_pin_x + nf * 3;
    if (h->Nf > 0) {
        PF_HIP(h, hipMemcpyAsync(h->d_pin_flags, dev_pin_flags, (size_t)h->Nf * 4, hipMemcpyDeviceToDevice, s));
        PF_HIP(h, hipMemcpyAsync(h->d_pin_x, dev_pin_x, (size_t)h->Nf * 3 * 4, hipMemcpyDeviceToDevice, s));
        PF_HIP(h, hipMemcpyAsync(h->d_pin_h, dev_pin_h, (size_t)h->Nf * nh * 4, hipMemcpyDeviceToDevice, s));
    }
    h->pin_feat_norm = feat_norm_constant;
    h->run = RUN_PINNED;
    return PF_OK;
}
int pf_sample_begin_pinned(pf_handle* h, const float* dev_init_pharm_com, const float* dev_noise0, const int32_t* dev_pin_flags,
                           const float* dev_pin_x, const float* dev_pin_h, float feat_norm_constant, pf_stream stream) {
    const bool seeded = h && take(h->seed_armed);
    if (const int rc = refuse_field(h, "pf_sample_begin_pinned")) return rc;
    return begin_pinned(h, dev_init_pharm_com, dev_noise0, dev_pin_flags, dev_pin_x, dev_pin_h, feat_norm_constant, seeded, stream);
}

// Arms the next begin with a seed (the semantics: pfdyn.h).  Every argument check runs before anything is touched; the two arrays
// become the handle's own (stream-ordered copies into run scratch), so a run in progress -- which reads none of it -- goes on
int pf_sample_seed_next(pf_handle* h, const pf_seed_coef* coef, const float* dev_seed_x, const float* dev_seed_h, float feat_norm_constant,
                        pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!coef || !dev_seed_x || !dev_seed_h) PF_FAIL(h, PF_ERR_ARG, "pf_sample_seed_next: null argument");
    if (!std::isfinite(coef->alpha_a) || !std::isfinite(coef->sigma_a) || !(coef->alpha_a > 0.f) || coef->sigma_a < 0.f)
        PF_FAIL(h, PF_ERR_ARG, "pf_sample_seed_next: alpha_a must be finite and > 0, sigma_a finite and >= 0");
    if (!(feat_norm_constant > 0.f) || !std::isfinite(feat_norm_constant)) PF_FAIL(h, PF_ERR_ARG, "pf_sample_seed_next: feat_norm_constant must be positive");
    hipStream_t s = (hipStream_t)stream;
    const size_t nf = (size_t)std::max(h->Nf, 1), nh = (size_t)h->cfg.pharm_nf;
    const size_t bytes = nf * 4 * (3 + nh);
    h->seed_armed = false;                  // (a seed armed before and not yet used is replaced, also when the copies below fail)
    PF_HIP(h, h->d_seed.reserve(bytes, bytes, Wait::on(s)));
    h->d_seed_x = h->d_seed.as<float>(); h->d_seed_h = h->d_seed_x + nf * 3;
    if (h->Nf > 0) {
        PF_HIP(h, hipMemcpyAsync(h->d_seed_x, dev_seed_x, (size_t)h->Nf * 3 * 4, hipMemcpyDeviceToDevice, s));
        PF_HIP(h, hipMemcpyAsync(h->d_seed_h, dev_seed_h, (size_t)h->Nf * nh * 4, hipMemcpyDeviceToDevice, s));
    }
    h->seed_alpha = coef->alpha_a; h->seed_sigma = coef->sigma_a; h->seed_feat_norm = feat_norm_constant;
    h->seed_armed = true;
    return PF_OK;
}

// One denoising step of a pinned run.  The dynamics call is sequenced WITHOUT a step (no tail, fused-tail or merged launch); the
// step ends with one launch of its own: the pinned update and, with the encoders on the fly, the generic edge build
int pf_denoise_step_pinned(pf_handle* h, const pf_step_coef* coef, const pf_pin_coef* pin, const float* dev_noise, int32_t ep_coord,
                           int32_t ep_feat, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!coef || !pin || !dev_noise) PF_FAIL(h, PF_ERR_ARG, "pf_denoise_step_pinned: null argument");
    if ((rc = run_guard(h, __func__, RUN_PINNED)) != PF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const StepParams sp = step_params(h, coef, dev_noise, ep_coord, ep_feat);
    StepMove mv;
    mv.args.kind = StepMoveArgs::PINNED; mv.args.pin = pin_params(h, pin);
    ++h->step_id;
    rc = run_dynamics(h, h->d_eps_h, h->d_eps_x, s, &coef->t, false, nullptr);
    if (rc) return rc;
    return step_end(h, sp, mv, s);
}

// Resampling jump of a pinned run: the whole state goes from level b back up to level a with one launch and no dynamics call
// (k_step_build<MoveRenoise>: the forward move + the generic edge build; k_step_update<MoveRenoise> where the next dynamics call builds its own edges)
int pf_renoise_step(pf_handle* h, const pf_renoise_coef* coef, const float* dev_noise, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!coef || !dev_noise) PF_FAIL(h, PF_ERR_ARG, "pf_renoise_step: null argument");
    if ((rc = run_guard(h, __func__, RUN_PINNED, true)) != PF_OK) return rc;
    const StepParams sp = step_params_base(h, dev_noise);
    StepMove mv;
    mv.args.kind = StepMoveArgs::RENOISE;
    mv.args.renoise.alpha_ts = coef->alpha_t_given_s; mv.args.renoise.sigma_ts = coef->sigma_t_given_s;
    ++h->step_id;
    return step_end(h, sp, mv, (hipStream_t)stream);
}

// One multistep step inside a plain run.  As in a pinned step the dynamics call is sequenced WITHOUT a step; the step ends with one
// launch of its own: the linear move, which also stores this step's outputs as the history, and, with the encoders on the fly, the
// generic edge build.  A non-zero c1 needs the outputs of a multistep step right in front of this one: refused before any launch
int pf_denoise_step_ms(pf_handle* h, const pf_ms_coef* coef, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!coef) PF_FAIL(h, PF_ERR_ARG, "pf_denoise_step_ms: null argument");
    if ((rc = run_guard(h, __func__, RUN_PLAIN)) != PF_OK) return rc;
    const float cs[6] = {coef->cz_x, coef->c0_x, coef->c1_x, coef->cz_h, coef->c0_h, coef->c1_h};
    for (float c : cs) if (!std::isfinite(c)) PF_FAIL(h, PF_ERR_ARG, "pf_denoise_step_ms: a coefficient is not finite");
    if ((coef->c1_x != 0.f || coef->c1_h != 0.f) && !h->ms_hist_valid)
        PF_FAIL(h, PF_ERR_STATE, "pf_denoise_step_ms: c1 != 0 needs the outputs of a multistep step right in front of this one (the first "
                                 "step of a run, and the first after any other move, must have c1 == 0)");
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)std::max(h->Nf, 1) * 4 * (3 + (size_t)h->cfg.pharm_nf);
    PF_HIP(h, h->d_ms_hist.reserve(bytes, bytes, Wait::on(s)));
    StepParams sp = step_params_base(h, nullptr);
    sp.eps_h = h->d_eps_h; sp.eps_x = h->d_eps_x;
    StepMove mv;
    mv.args.kind = StepMoveArgs::MS;
    MsParams& q = mv.args.ms;
    q.hist = h->d_ms_hist.as<float>();
    q.cz_x = coef->cz_x; q.c0_x = coef->c0_x; q.c1_x = coef->c1_x; q.cz_h = coef->cz_h; q.c0_h = coef->c0_h; q.c1_h = coef->c1_h;
    ++h->step_id;
    rc = run_dynamics(h, h->d_eps_h, h->d_eps_x, s, &coef->t, false, nullptr);
    if (rc) return rc;
    return step_end(h, sp, mv, s);
}

int pf_prepare_timesteps(pf_handle* h, const float* host_t, int32_t n, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (n < 0 || (n && !host_t)) PF_FAIL(h, PF_ERR_ARG, "pf_prepare_timesteps: bad argument");
    h->t_plan.assign(host_t, host_t + n); h->plan_pos = 0;   // (a denoising step finds the NEXT call's timestep here: center hoist)
    if (n > L0_PTAB_SLOTS - 64) n = L0_PTAB_SLOTS - 64;      // the rest are computed when their steps arrive
    if (l0_hoist_ok(h)) l0_prepare_t(h, host_t, n, (hipStream_t)stream);
    return PF_OK;
}

int pf_sample_frame(pf_handle* h, float feat_norm_constant, float* dev_x, float* dev_h, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if ((rc = run_guard(h, __func__, RUN_NONE)) != PF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    pfk_segment_mean(h->d_xn, h->d_prot_ptr, 0, h->B, h->d_com_tmp, s);
    if (dev_x) pfk_export_coords(h->d_xn, h->Np, h->Nf, h->d_gid, h->d_com_init, h->d_com_tmp, dev_x, s);
    if (dev_h) pfk_scale_copy(h->d_pharm_h, dev_h, (size_t)h->Nf * h->cfg.pharm_nf, feat_norm_constant, s);
    return PF_OK;
}

// a pinned (or guided) run returns the given values bit for bit: x_0 / h_0 and the last trajectory frame
static void pin_restore(pf_handle* h, float* dev_x, float* dev_h, pf_stream stream) {
    if (h->run >= RUN_PINNED) pfk_pin_restore(h->d_pin_flags, h->d_pin_x, h->d_pin_h, h->Nf, h->cfg.pharm_nf, dev_x, dev_h, (hipStream_t)stream);
}

int pf_sample_end(pf_handle* h, float feat_norm_constant, float* dev_x0, float* dev_h0, pf_stream stream) {
    // x_0 = x_t - protein COM + initial protein COM ; h_0 = h_t * norm constant  (pharmacodiff.py:480-488)
    int rc = pf_sample_frame(h, feat_norm_constant, dev_x0, dev_h0, stream);
    if (rc == PF_OK) pin_restore(h, dev_x0, dev_h0, stream);
    // the exchange's cumulative time-out count travels with the results: once the caller has waited for x_0 / h_0 it is on
    // the host too, and pf_sample_status judges THIS run without touching the device
    if (rc == PF_OK && h->d_xstat)
        PF_HIP(h, hipMemcpyAsync(h->xstat_host, h->d_xstat, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return rc;
}

int pf_sample_status(pf_handle* h, int32_t* n_timeouts) {
    if (!h) return PF_ERR_ARG;
    if (n_timeouts) *n_timeouts = 0;
    if (!h->xstat_host) return PF_OK;
    const int seen = *(volatile int*)h->xstat_host;
    if (seen == h->xstat_ack) return PF_OK;
    const int n = seen - h->xstat_ack;
    h->xstat_ack = seen;
    if (n_timeouts) *n_timeouts = n;
    h->pol.hs_build = 0;                    // this handle goes on with the separate launches
    PF_FAIL(h, PF_ERR_EXCHANGE, "%d time-out(s) in the exchange of the merged last launch (k_rg_node_hs_build): the sampling run(s) that "
                                "ended since the last status call are invalid and must be repeated; the handle now uses the separate "
                                "node + head and update + build launches", n);
}

int pf_debug_xchg_fault(pf_handle* h, int32_t drop_word, int32_t poll_max) {
    if (!h) return PF_ERR_ARG;
    h->xchg_fault = drop_word ? 1 : 0;
    h->xchg_poll_max = poll_max > 0 ? poll_max : 0;
    return PF_OK;
}

// One whole run, as the four pf_sample* entry points describe it.  kind: which begin and which step; op: NULL (every op is a
// denoising step) or per op 0 (a step) / 1 (a resampling jump); the coefficient arrays have one entry per op, read where the
// op's kind needs it; pin_*: RUN_PINNED and RUN_GUIDED; restr_* / guide_*: RUN_GUIDED; traj_* / energy: optional outputs
struct SampleRun {
    RunKind kind; int32_t n_ops; const int32_t* op;
    const pf_step_coef* coef; const pf_pin_coef* pin_coef; const pf_renoise_coef* renoise; const pf_guide_coef* guide_coef;
    const pf_ms_coef* ms_coef;              // RUN_PLAIN only: every op is a multistep step, and noise is the initial draw alone
    const float *noise, *com;
    const int32_t* pin_flags; const float *pin_x, *pin_h;
    const int32_t *restr_ptr, *restr_kind, *restr_center; const float *restr_p, *restr_r, *restr_w; float guide_scale, guide_clip;
    int32_t ep_coord, ep_feat; float feat_norm;
    float *x0, *h0, *traj_x, *traj_h, *energy;
};
// the whole loop of pf_sample / pf_sample_pinned / pf_sample_pinned_resampled / pf_sample_guided
static int sample_loop(pf_handle* h, const SampleRun& r, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    const bool pinned = r.kind >= RUN_PINNED, guided = r.kind == RUN_GUIDED;
    const int n_ops = r.n_ops;
    const bool ms = r.ms_coef != nullptr;
    if (n_ops < 0 || (n_ops && ((!r.coef && !ms) || (guided && (!r.pin_coef || !r.guide_coef)))) || !r.noise)
        PF_FAIL(h, PF_ERR_ARG, "%s: bad argument", guided ? "pf_sample_guided" : ms ? "pf_sample_ms" : "pf_sample");
    if (pinned && n_ops && !r.pin_coef) PF_FAIL(h, PF_ERR_ARG, "pf_sample_pinned: null host_pin_coef");
    for (int i = 0; r.op && i < n_ops; ++i) {
        if (r.op[i] != 0 && r.op[i] != 1) PF_FAIL(h, PF_ERR_ARG, "pf_sample_pinned_resampled: op %d has kind %d (0 denoise, 1 renoise)", i, (int)r.op[i]);
        if (r.op[i] == 1 && !r.renoise) PF_FAIL(h, PF_ERR_ARG, "pf_sample_pinned_resampled: null host_renoise");
    }
    const size_t row = (size_t)h->Nf * (3 + h->cfg.pharm_nf);
    const size_t fx = (size_t)h->Nf * 3, fh = (size_t)h->Nf * h->cfg.pharm_nf;
    if (guided) rc = pf_sample_begin_guided(h, r.com, r.noise, r.pin_flags, r.pin_x, r.pin_h, r.feat_norm, r.restr_ptr, r.restr_kind, r.restr_center,
                                            r.restr_p, r.restr_r, r.restr_w, r.guide_scale, r.guide_clip, stream);
    else if (pinned) rc = pf_sample_begin_pinned(h, r.com, r.noise, r.pin_flags, r.pin_x, r.pin_h, r.feat_norm, stream);
    else rc = pf_sample_begin(h, r.com, r.noise, stream);
    if (rc) return rc;
    const bool traj = r.traj_x || r.traj_h;
    auto frame = [&](int i) { return pf_sample_frame(h, r.feat_norm, r.traj_x ? r.traj_x + (size_t)i * fx : nullptr, r.traj_h ? r.traj_h + (size_t)i * fh : nullptr, stream); };
    if (traj && (rc = frame(0)) != PF_OK) return rc;
    if (!guided) {      // (a guided step's dynamics call is a training forward: nothing is hoisted or computed ahead for it)
        std::vector<float> tv;                  // the denoising steps' timesteps in op order
        tv.reserve(n_ops);
        for (int i = 0; i < n_ops; ++i) if (!r.op || r.op[i] == 0) tv.push_back(ms ? r.ms_coef[i].t : r.coef[i].t);
        rc = pf_prepare_timesteps(h, tv.data(), (int32_t)tv.size(), stream);
        if (rc) return rc;
    }
    for (int i = 0; i < n_ops; ++i) {
        // this op's noise row; a multistep run has the initial draw alone and reads no other
        const float* nz = ms ? nullptr : r.noise + (size_t)(i + 1) * row;
        if (ms) rc = pf_denoise_step_ms(h, r.ms_coef + i, stream);
        else if (r.op && r.op[i] == 1) rc = pf_renoise_step(h, r.renoise + i, nz, stream);
        else if (guided) {
            h->guide_traj_energy = r.energy ? r.energy + (size_t)i * h->B : nullptr;
            rc = pf_denoise_step_guided(h, r.coef + i, r.pin_coef + i, r.guide_coef + i, nz, r.ep_coord, r.ep_feat, stream);
            h->guide_traj_energy = nullptr;
        } else rc = pinned ? pf_denoise_step_pinned(h, r.coef + i, r.pin_coef + i, nz, r.ep_coord, r.ep_feat, stream)
                           : pf_denoise_step(h, r.coef + i, nz, r.ep_coord, r.ep_feat, stream);
        if (rc) return rc;
        if (traj && (rc = frame(i + 1)) != PF_OK) return rc;
    }
    // the last frame of a pinned run carries the given values like x_0 / h_0 do (frame n_ops == x_0 / h_0, as in unpinned runs)
    pin_restore(h, r.traj_x ? r.traj_x + (size_t)n_ops * fx : nullptr, r.traj_h ? r.traj_h + (size_t)n_ops * fh : nullptr, stream);
    return pf_sample_end(h, r.feat_norm, r.x0, r.h0, stream);
}

int pf_sample(pf_handle* h, int32_t n_steps, const pf_step_coef* host_coef, const float* dev_noise,
              const float* dev_init_pharm_com, int32_t ep_coord, int32_t ep_feat, float feat_norm_constant,
              float* dev_x0, float* dev_h0, float* dev_traj_x, float* dev_traj_h, pf_stream stream) {
    SampleRun r{};
    r.kind = RUN_PLAIN; r.n_ops = n_steps; r.coef = host_coef; r.noise = dev_noise; r.com = dev_init_pharm_com;
    r.ep_coord = ep_coord; r.ep_feat = ep_feat; r.feat_norm = feat_norm_constant;
    r.x0 = dev_x0; r.h0 = dev_h0; r.traj_x = dev_traj_x; r.traj_h = dev_traj_h;
    return sample_loop(h, r, stream);
}

int pf_sample_ms(pf_handle* h, int32_t n_steps, const pf_ms_coef* host_coef, const float* dev_noise0, const float* dev_init_pharm_com,
                 float feat_norm_constant, float* dev_x0, float* dev_h0, float* dev_traj_x, float* dev_traj_h, pf_stream stream) {
    if (h && n_steps > 0 && !host_coef) PF_FAIL(h, PF_ERR_ARG, "pf_sample_ms: null host_coef");
    static const pf_ms_coef none{};
    SampleRun r{};
    r.kind = RUN_PLAIN; r.n_ops = n_steps; r.ms_coef = host_coef ? host_coef : &none; r.noise = dev_noise0; r.com = dev_init_pharm_com;
    r.feat_norm = feat_norm_constant;
    r.x0 = dev_x0; r.h0 = dev_h0; r.traj_x = dev_traj_x; r.traj_h = dev_traj_h;
    return sample_loop(h, r, stream);
}

int pf_sample_pinned_resampled(pf_handle* h, int32_t n_ops, const int32_t* host_op, const pf_step_coef* host_coef, const pf_pin_coef* host_pin_coef,
                               const pf_renoise_coef* host_renoise, const float* dev_noise, const float* dev_init_pharm_com,
                               const int32_t* dev_pin_flags, const float* dev_pin_x, const float* dev_pin_h, int32_t ep_coord, int32_t ep_feat,
                               float feat_norm_constant, float* dev_x0, float* dev_h0, float* dev_traj_x, float* dev_traj_h, pf_stream stream) {
    if (h && (!dev_pin_flags || !dev_pin_x || !dev_pin_h)) PF_FAIL(h, PF_ERR_ARG, "pf_sample_pinned_resampled: null pin array");
    if (h && n_ops > 0 && !host_op) PF_FAIL(h, PF_ERR_ARG, "pf_sample_pinned_resampled: null host_op");
    SampleRun r{};
    r.kind = RUN_PINNED; r.n_ops = n_ops; r.op = host_op; r.coef = host_coef; r.pin_coef = host_pin_coef; r.renoise = host_renoise;
    r.noise = dev_noise; r.com = dev_init_pharm_com; r.pin_flags = dev_pin_flags; r.pin_x = dev_pin_x; r.pin_h = dev_pin_h;
    r.ep_coord = ep_coord; r.ep_feat = ep_feat; r.feat_norm = feat_norm_constant;
    r.x0 = dev_x0; r.h0 = dev_h0; r.traj_x = dev_traj_x; r.traj_h = dev_traj_h;
    return sample_loop(h, r, stream);
}

int pf_sample_pinned(pf_handle* h, int32_t n_steps, const pf_step_coef* host_coef, const pf_pin_coef* host_pin_coef, const float* dev_noise,
                     const float* dev_init_pharm_com, const int32_t* dev_pin_flags, const float* dev_pin_x, const float* dev_pin_h,
                     int32_t ep_coord, int32_t ep_feat, float feat_norm_constant, float* dev_x0, float* dev_h0,
                     float* dev_traj_x, float* dev_traj_h, pf_stream stream) {
    if (h && (!dev_pin_flags || !dev_pin_x || !dev_pin_h)) PF_FAIL(h, PF_ERR_ARG, "pf_sample_pinned: null pin array");
    SampleRun r{};
    r.kind = RUN_PINNED; r.n_ops = n_steps; r.coef = host_coef; r.pin_coef = host_pin_coef;
    r.noise = dev_noise; r.com = dev_init_pharm_com; r.pin_flags = dev_pin_flags; r.pin_x = dev_pin_x; r.pin_h = dev_pin_h;
    r.ep_coord = ep_coord; r.ep_feat = ep_feat; r.feat_norm = feat_norm_constant;
    r.x0 = dev_x0; r.h0 = dev_h0; r.traj_x = dev_traj_x; r.traj_h = dev_traj_h;
    return sample_loop(h, r, stream);
}

// ---- scoring: the per-level terms of the variational bound for GIVEN pharmacophores (include/pfdyn.h: pf_score) ----
// A level is k_score_prepare + the inference forward at the uniform timestep t_int / T + k_score_eval (pf_score.hip).  The pocket
// of every graph is the bound one translated rigidly (by the two COMs of its candidate), as in a sampling run: conv layer 0's
// pocket-side constants (zs: functions of coordinate DIFFERENCES inside one pocket) hold for every level, and so does a
// pocket-group claim -- coords_custom stays false, as behind pf_sample_begin.  They are made anew once per call and dropped
// behind it, so that the call's bits depend on its arguments alone and a later run's on its own.
int pf_score(pf_handle* h, const float* dev_pharm_x0, const float* dev_pharm_h0, int32_t n_levels, const pf_score_level* host_levels,
             const float* dev_noise, const float* dev_alpha, const float* dev_sigma, int32_t n_timesteps, float feat_norm,
             int32_t remove_com, int32_t endpoint_param_coord, int32_t endpoint_param_feat, float* dev_score, float* dev_terms,
             pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (h->run != RUN_NONE)
        PF_FAIL(h, PF_ERR_STATE, "pf_score inside a %s run (%s): the run's state is the handle's; bind the batch again to end the run", RUN_ROWS[h->run].name,
                RUN_ROWS[h->run].begin);
    if (!dev_pharm_x0 || !dev_pharm_h0 || !host_levels || !dev_noise || !dev_alpha || !dev_sigma || !dev_score) PF_FAIL(h, PF_ERR_ARG, "pf_score: null argument");
    if (n_levels < 1) PF_FAIL(h, PF_ERR_ARG, "pf_score: n_levels %d (at least one level)", (int)n_levels);
    if (n_timesteps < 1 || !(feat_norm > 0.f)) PF_FAIL(h, PF_ERR_ARG, "pf_score: bad n_timesteps / feat_norm");
    for (int l = 0; l < n_levels; ++l)
        if (host_levels[l].t_int < 0 || host_levels[l].t_int > n_timesteps)
            PF_FAIL(h, PF_ERR_ARG, "pf_score: level %d has t_int %d outside 0..%d", l, (int)host_levels[l].t_int, (int)n_timesteps);
    if (h->Nf == 0) PF_FAIL(h, PF_ERR_ARG, "pf_score: the batch has no pharmacophore centers (nothing to score)");
    if (h->cfg.pharm_nf > 8) PF_FAIL(h, PF_ERR_ARG, "pf_score: pharm_nf %d (the evaluation kernel holds at most 8 feature columns)", (int)h->cfg.pharm_nf);
    // a pocket-group claim about DEVICE rows: its verdict is read here (the wait the first sharing call makes anyway), so that a false
    // claim too is refused before anything is launched
    if (h->share_ok && h->share_check == 0) (void)share_now(h);
    if (h->share_check == 2)
        PF_FAIL(h, PF_ERR_ARG, "pf_set_pocket_groups: the claim made for this batch is false -- a graph differs from its representative in "
                               "coordinates or features (compared on the device); bind the batch again without the claim");
    hipStream_t s = (hipStream_t)stream;
    // a kept training forward does not survive: every level overwrites the coordinates and dynamic edges its backward reads again
    h->t_have_fwd = false; h->t_have_loss = false;
    h->coords_custom = false; h->zs_batch_coords = false;
    std::vector<float> tv((size_t)n_levels);
    for (int l = 0; l < n_levels; ++l) tv[l] = (float)host_levels[l].t_int / (float)n_timesteps;
    // conv layer 0's per-timestep tables of every level up front, 64 timesteps per launch (the resident cache holds L0_PTAB_SLOTS: what is
    // beyond is computed when its level arrives); the sampler's plan (pf_prepare_timesteps' other half) is not this call's to set
    if (l0_hoist_ok(h)) l0_prepare_t(h, tv.data(), std::min<int>(n_levels, L0_PTAB_SLOTS - 64), s);
    ScoreParams sp{};
    sp.B = h->B; sp.Np = h->Np; sp.nf = h->cfg.pharm_nf; sp.remove_com = remove_com != 0; sp.feat_norm = feat_norm;
    sp.prot_ptr = h->d_prot_ptr; sp.pharm_ptr = h->d_pharm_ptr; sp.prot_x0 = h->d_prot_x0;
    sp.x0 = dev_pharm_x0; sp.h0 = dev_pharm_h0; sp.alpha_tab = dev_alpha; sp.sigma_tab = dev_sigma;
    sp.xn = h->d_xn; sp.pharm_h = h->d_pharm_h; sp.dyn_h = h->d_eps_h; sp.dyn_x = h->d_eps_x; sp.score = dev_score;
    const size_t row = (size_t)h->Nf * (3 + h->cfg.pharm_nf);
    for (int l = 0; l < n_levels && rc == PF_OK; ++l) {
        sp.t_int = host_levels[l].t_int; sp.w_pos = host_levels[l].w_pos; sp.w_feat = host_levels[l].w_feat; sp.first = l == 0;
        sp.noise = dev_noise + (size_t)l * row;
        sp.terms = dev_terms ? dev_terms + (size_t)l * h->B * 4 : nullptr;
        h->edges_built = false; h->rec_valid = false;      // the centers moved, and each pocket with them
        { ProfScope ps(h, pf_handle::K_STEP, s); pfk_score_prepare(&sp, s); }      // (class 5 of pf_profile_read: what a level adds to its forward)
        rc = run_dynamics(h, h->d_eps_h, h->d_eps_x, s, &tv[l], false);
        if (rc == PF_OK) { ProfScope ps(h, pf_handle::K_STEP, s); pfk_score_eval(&sp, endpoint_param_coord != 0, endpoint_param_feat != 0, s); }
    }
    // the handle holds the bound coordinates again, as the bind left them
    pfk_load_coords(h->d_prot_x0, h->d_xn, h->Np, h->d_gid, nullptr, 0.f, s);
    h->edges_built = false; h->rec_valid = false; h->zs_batch_coords = false;
    if (rc) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return PF_OK;
}

int64_t pf_debug_get_edges(pf_handle* h, int32_t etype, int32_t* host_src, int32_t* host_dst, int64_t capacity,
                           pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (etype < 0 || etype > 3) PF_FAIL(h, PF_ERR_ARG, "bad etype");
    hipStream_t s = (hipStream_t)stream;
    PF_HIP(h, hipStreamSynchronize(s));
    const int B = h->B, Np = h->Np;
    std::vector<int> cnt((size_t)3 * B);
    PF_HIP(h, hipMemcpy(cnt.data(), h->d_dyn_cnt, (size_t)3 * B * 4, hipMemcpyDeviceToHost));
    int64_t total = 0;
    if (etype == ET_PP) total = h->Epp;
    else for (int g = 0; g < B; ++g) total += cnt[(size_t)etype * B + g];
    if (!host_src || !host_dst) return total;
    if (capacity < total) PF_FAIL(h, PF_ERR_ARG, "capacity too small");
    std::vector<int> es(std::max<int64_t>(h->Ecap, 1)), ed(std::max<int64_t>(h->Ecap, 1));
    PF_HIP(h, hipMemcpy(es.data(), h->d_esrc, (size_t)h->Ecap * 4, hipMemcpyDeviceToHost));
    PF_HIP(h, hipMemcpy(ed.data(), h->d_edst, (size_t)h->Ecap * 4, hipMemcpyDeviceToHost));
    const bool src_pharm = (etype == ET_FF || etype == ET_FP), dst_pharm = (etype == ET_FF || etype == ET_PF);
    int64_t o = 0;
    auto emit = [&](int64_t a, int64_t n) {
        for (int64_t e = a; e < a + n; ++e, ++o) {
            host_src[o] = es[e] - (src_pharm ? Np : 0);
            host_dst[o] = ed[e] - (dst_pharm ? Np : 0);
        }
    };
    if (etype == ET_PP) emit(0, h->Epp);
    else for (int g = 0; g < B; ++g) emit(h->h_reg[(size_t)etype * B + g], cnt[(size_t)etype * B + g]);
    return total;
}

int pf_debug_conv_layer(pf_handle* h, int32_t layer, const float* dev_prot_x, const float* dev_pharm_x,
                        const float* hp_, const float* vp_, const float* hf_, const float* vf_,
                        float* ohp, float* ovp, float* ohf, float* ovf, pf_stream stream) {
    if (h && !h->spec) PF_FAIL(h, PF_ERR_ARG, "%s: specialised to n_hidden_scalars 128 / vector_size 16", __func__);
    int rc = check_ready(h, true);
    if (rc) return rc;
    const pf_config& c = h->cfg;
    if (layer < 0 || layer >= c.n_convs) PF_FAIL(h, PF_ERR_ARG, "bad layer");
    hipStream_t s = (hipStream_t)stream;
    load_state(h, dev_prot_x, dev_pharm_x, nullptr, s);
    const size_t Np = h->Np, Nf = h->Nf;
    pfk_copy(hp_, h->d_h[0], Np * PF_S, s);
    pfk_copy(hf_, h->d_h[0] + Np * PF_S, Nf * PF_S, s);
    pfk_copy(vp_, h->d_v[0], Np * 48, s);
    pfk_copy(vf_, h->d_v[0] + Np * 48, Nf * 48, s);
    BuildParams bp{};       // (not build_params(): it would add eorig, act_ids of a pruned model and, in a sampling run, pa_stamp)
    bp.B = h->B; bp.Np_tot = h->Np; bp.prot_ptr = h->d_prot_ptr; bp.pharm_ptr = h->d_pharm_ptr; bp.xn = h->d_xn;
    bp.reg = h->d_reg; bp.dyn_cnt = h->d_dyn_cnt; bp.esrc = h->d_esrc; bp.edst = h->d_edst;
    bp.in_start = h->d_in_start; bp.in_cnt = h->d_in_cnt; bp.N = h->N; bp.ff_k = c.ff_k; bp.pf_k = c.pf_k;
    bp.r2_ff = c.cutoff_ff * c.cutoff_ff; bp.r2_pf = c.cutoff_pf * c.cutoff_pf;
    bp.gnorm = h->d_gnorm; bp.pp_cnt = h->d_pp_cnt; bp.pfq_cnt = h->d_pfq_cnt; bp.norm_mode = c.message_norm_mode;
    bp.act_ids = nullptr; bp.reg_act = h->d_reg_act;
    pfk_build_edges(&bp, s);
    EdgeParams e = edge_params_base(h, layer, false, false);      // the dense tile lists, whichever layer
    e.h = h->d_h[0]; e.v = h->d_v[0]; e.msg_s = h->d_msg_s; e.msg_v = h->d_msg_v;
    const int rg = h->pol.rg_mode(e.ntiles);                  // same choice as run_dynamics
    if (rg) pfk_rg_edge(&e, nullptr, 0, rg, 0, 0, s);
    else if (e.ntiles <= h->pol.coop_edge_max) pfk_edge_msg_coop(&e, 0, s); else pfk_edge_msg(&e, 0, s);
    NodeParams n = node_params_base(h, layer, false, false);
    n.msg_s = h->d_msg_s; n.msg_v = h->d_msg_v; n.h_in = h->d_h[0]; n.v_in = h->d_v[0]; n.h_out = h->d_h[1]; n.v_out = h->d_v[1];
    n.grp = n.grp_pa = rg ? 4 * rg : 32;
    if (rg) pfk_rg_node(&n, nullptr, nullptr, 0, std::max(1, h->pol.rg_mode(n.ntiles)), 0, s);
    else if (n.ntiles <= h->pol.coop_node_max) pfk_node_update_coop(&n, 0, s); else pfk_node_update(&n, 0, s);
    pfk_copy(h->d_h[1], ohp, Np * PF_S, s);
    pfk_copy(h->d_h[1] + Np * PF_S, ohf, Nf * PF_S, s);
    pfk_copy(h->d_v[1], ovp, Np * 48, s);
    pfk_copy(h->d_v[1] + Np * 48, ovf, Nf * 48, s);
    // the zero-vector invariant of buffer 0 (layer-0 kernels never read it, later layers overwrite it)
    PF_HIP(h, hipMemsetAsync(h->d_v[0], 0, (size_t)h->N * 48 * 4, s));
    hipError_t er = hipGetLastError();
    if (er != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(er));
    return PF_OK;
}

// ------------------------------------------------------------------------------------------------
// gradient path (training step): forward that keeps the per-layer state, backward, parameter layout
// ------------------------------------------------------------------------------------------------
// what the gradient kernels of both legs are built for: PF_OK, or the error
static int train_limits_ok(pf_handle* h) {
    const pf_config& c = h->cfg;
    if (c.n_message_gvps > PFT_MAX_CHAIN || c.n_noise_gvps > PFT_MAX_CHAIN || c.n_update_gvps > 3)
        PF_FAIL(h, PF_ERR_ARG, "training supports at most %d message / noise GVPs and 3 update GVPs per chain", PFT_MAX_CHAIN);
    if (c.pharm_nf > 8 || c.rec_nf + 1 > 17 || c.pharm_nf + 1 > 17)
        PF_FAIL(h, PF_ERR_ARG, "training supports pharm_nf <= 8 and rec_nf <= 16");
    return PF_OK;
}
// floats between two gradient copies: the parameter count rounded up to a multiple of 64 (16-byte aligned rows)
static size_t grad_stride(const pf_handle* h) { return (h->nparams + 63) / 64 * 64; }
// an element is dropped iff its hash is below p * 2^32 (pf_drop_hash; 0: no dropout)
static bool dropout_ok(float p) { return p >= 0.f && p < 1.f; }
static uint32_t drop_threshold(float p) { return p > 0.f ? (uint32_t)std::min(4294967295.0, (double)p * 4294967296.0) : 0u; }

static int ensure_train_ws(pf_handle* h, hipStream_t s) {
    if (h->d_tws && h->t_ws_ready) return PF_OK;
    const pf_config& c = h->cfg;
    if (const int rc = train_limits_ok(h)) return rc;
    const int L = c.n_convs, N = h->N;
    const size_t E1 = (size_t)h->Ecap + 1, Es = (size_t)std::max<int64_t>(h->Ecap, 1), Nf1 = (size_t)std::max(h->Nf, 1);
    const size_t ng = (size_t)c.n_message_gvps, nu = (size_t)c.n_update_gvps, nh = (size_t)c.n_noise_gvps;
    h->t_nblk = std::max(8, std::min(256, h->n_edge_tiles));
    h->t_clist_cap = (size_t)std::max(h->n_edge_tiles, h->n_edge_tiles_act) * 32 + 64;
    h->t_ucap = 32 * std::max(h->n_node_tiles, h->n_node_tiles_act) + 16;      // rows per node type in the dense unit list
    h->t_ulist_cap = (size_t)2 * 2 * h->t_ucap + 64;
    h->wt_ready = false;                         // (the loss buffers t_l* below are shared with the width-generic leg's carve)
    h->t_H.assign(L + 1, nullptr); h->t_V.assign(L + 1, nullptr); h->t_msg_s.assign(L, nullptr); h->t_msg_v.assign(L, nullptr);
    h->t_nsv_z.assign(L, nullptr); h->t_nsv_g.assign(L, nullptr); h->t_nsv_v.assign(L, nullptr);
    h->t_sv_z.assign(L, nullptr); h->t_sv_g.assign(L, nullptr); h->t_sv_v.assign(L, nullptr);
    // two passes over one list: sizes, then pointers
    bool fresh = false;
    size_t bytes = 0;
    for (int pass = 0; pass < 2; ++pass) {
        Carver w(pass ? h->d_tws.get() : nullptr);
        for (int l = 0; l <= L; ++l) { w.take(h->t_H[l], (size_t)N * PF_S); w.take(h->t_V[l], (size_t)N * 48); }
        for (int l = 0; l < L; ++l) { w.take(h->t_msg_s[l], E1 * PF_S); w.take(h->t_msg_v[l], E1 * 48); }
        for (int a = 0; a < 2; ++a) { w.take(h->t_G_h[a], (size_t)N * PF_S); w.take(h->t_G_v[a], (size_t)N * 48); }
        w.take(h->t_gagg_s, (size_t)N * PF_S); w.take(h->t_gagg_v, (size_t)N * 48);
        w.take(h->t_fix, 64);
        w.take(h->t_ccnt, 128);                                 // [layer][16]: passes per etype, rows per etype at + 8; node units at [96]
        w.take(h->t_clist, h->t_clist_cap * L);                 // dense row lists, one per conv layer
        w.take(h->t_gpart_enc, (size_t)PFT_ENC_BLOCKS * std::max(h->enc_n, 1));
        w.take(h->t_ulist, h->t_ulist_cap * L);                 // per conv layer: [2 types][t_ucap] x (node id, saved-level row)
        w.take(h->t_Gg, (size_t)h->B * c.rec_nf * PF_S);
        w.take(h->t_lx0c, (size_t)h->Nf * 3); w.take(h->t_lag, (size_t)h->B); w.take(h->t_lsg, (size_t)h->B); w.take(h->t_lcom2, (size_t)h->B * 3);
        w.take(h->t_lgx, (size_t)h->Nf * 3); w.take(h->t_lgh, (size_t)h->Nf * c.pharm_nf); w.take(h->t_lout, 64);      // loss buffers
        for (int l = 0; l < L; ++l) { w.take(h->t_nsv_z[l], nu * 2 * N * PF_S); w.take(h->t_nsv_g[l], nu * 2 * N * 16); w.take(h->t_nsv_v[l], nu * 2 * N * 48); }
        w.take(h->t_hsv_z, nh * Nf1 * PF_S); w.take(h->t_hsv_g, nh * Nf1 * 16); w.take(h->t_hsv_v, nh * Nf1 * 48);
        w.take(h->t_gpart, (size_t)h->t_nblk * grad_stride(h));
        for (int l = 0; l < L; ++l) { w.take(h->t_sv_z[l], ng * Es * PF_S); w.take(h->t_sv_g[l], ng * Es * 16); w.take(h->t_sv_v[l], ng * Es * 48); }
        w.take(h->t_gs_buf, Es * PF_S); w.take(h->t_gv_buf, Es * 48);
        if (pass == 0) {
            // like d_ws the allocation outlives the batch: a training loop binds a new batch every step, and a free / allocate
            // pair of a few GB (plus clearing it) per step cost two orders of magnitude more than the step itself
            bytes = w.bytes();
            PF_HIP(h, h->d_tws.reserve(bytes + 4096, bytes + bytes / 8 + 4096, Wait::device(), &fresh));
        } else if (w.bytes() != bytes)
            PF_FAIL(h, PF_ERR_STATE, "training workspace: carved %zu bytes, counted %zu", w.bytes(), bytes);
    }
    {
        // int64 accumulators [N][128] and [N][48]: cleared when allocated, pfk_fix_apply leaves every element it read at zero
        const size_t a_bytes = ((size_t)N * PF_S * 8 + 255) / 256 * 256, need_a = a_bytes + (size_t)N * 48 * 8;
        PF_HIP(h, h->d_tA.reserve(need_a, need_a + need_a / 8, Wait::device(), &h->tA_dirty));
        if (h->tA_dirty) { PF_HIP(h, hipMemsetAsync(h->d_tA.get(), 0, h->d_tA.capacity(), s)); h->tA_dirty = false; }
        h->t_A_h = h->d_tA.as<long long>();
        h->t_A_v = reinterpret_cast<long long*>(h->d_tA.as<char>() + a_bytes);
    }
    // message buffers: the zero row (index Ecap) must read as zeros; V[0] is the all-zero initial vector state
    // (only rows written by the same forward and the zero row are ever read: a reused allocation needs just that row)
    {
        ZeroBatch zb(s);
        for (int l = 0; l < L; ++l) {
            if (fresh) {
                zb.add(h->t_msg_s[l], E1 * PF_S * 4);
                zb.add(h->t_msg_v[l], E1 * 48 * 4);
            } else {
                zb.add(h->t_msg_s[l] + (E1 - 1) * PF_S, PF_S * 4);
                zb.add(h->t_msg_v[l] + (E1 - 1) * 48, 48 * 4);
            }
        }
        zb.add(h->t_V[0], (size_t)N * 48 * 4);
        zb.flush();
    }
    h->t_ws_ready = true;
    return PF_OK;
}


// workspace of the width-generic training leg (pf_train_set_family): what k_wide_edge<true> / k_wide_node<true> keep, the gradient
// buffers of pf_wide_train.hip, the gradient copies and the loss buffers
static int ensure_wide_train_ws(pf_handle* h, hipStream_t s) {
    if (h->d_wtws && h->wt_ready) return PF_OK;
    const pf_config& c = h->cfg;
    if (const int rc = train_limits_ok(h)) return rc;
    const size_t L = c.n_convs, N = h->N, S = c.n_hidden_scalars, V3 = (size_t)3 * c.vector_size;
    const size_t ES = S + PF_R, EV = V3 + 3, Es = (size_t)std::max<int64_t>(h->Ecap, 1), Nf1 = (size_t)std::max(h->Nf, 1);
    const size_t nm = c.n_message_gvps, nu = c.n_update_gvps, nh = c.n_noise_gvps;
    const size_t gstride = grad_stride(h);
    pf_handle::WtWs& w = h->wt;
    // two passes over one list: sizes, then pointers
    size_t bytes = 0;
    for (int pass = 0; pass < 2; ++pass) {
        Carver cv(pass ? h->d_wtws.get() : nullptr);
        auto take = [&](float*& dst, size_t n) { cv.take(dst, n); };
        take(w.esv_s, L * nm * Es * ES); take(w.esv_v, L * nm * Es * EV);
        take(w.x1_s, L * N * S); take(w.x1_v, L * N * V3); take(w.x2_s, L * N * S); take(w.x2_v, L * N * V3);
        take(w.usv_s, L * nu * N * S); take(w.usv_v, L * nu * N * V3);
        take(w.hsv_s, nh * Nf1 * S); take(w.hsv_v, nh * Nf1 * V3); take(w.h64, Nf1 * 64);
        for (int a = 0; a < 2; ++a) { take(w.G_s[a], N * S); take(w.G_v[a], N * V3); }
        take(w.gch_s, N * S); take(w.gch_v, N * V3); take(w.gres_s, N * S); take(w.gres_v, N * V3);
        take(w.gagg_s, N * S); take(w.gagg_v, N * V3);
        take(w.ges, Es * ES); take(w.gev, Es * EV);
        take(w.xkeep, N * 4); take(w.gdiff, L * Es * 3);
        take(w.gpart, (size_t)PFWT_NB * gstride); take(w.fix, 64);
        for (int a = 0; a < 2; ++a) { take(w.st_h[a], N * S); take(w.st_v[a], N * V3); }
        take(w.msg_s, Es * S); take(w.msg_v, Es * V3);
        take(h->t_lx0c, (size_t)h->Nf * 3); take(h->t_lag, (size_t)h->B); take(h->t_lsg, (size_t)h->B); take(h->t_lcom2, (size_t)h->B * 3);
        take(h->t_lgx, (size_t)h->Nf * 3); take(h->t_lgh, (size_t)h->Nf * c.pharm_nf); take(h->t_lout, 64);
        if (pass == 0) {
            bytes = cv.bytes();
            PF_HIP(h, h->d_wtws.reserve(bytes + 4096, bytes + bytes / 8 + 4096, Wait::device()));
        } else if (cv.bytes() != bytes)
            PF_FAIL(h, PF_ERR_STATE, "width-generic training workspace: carved %zu bytes, counted %zu", cv.bytes(), bytes);
    }
    w.Es = Es;
    const size_t a_bytes = (N * S * 8 + 255) / 256 * 256, need_a = a_bytes + N * V3 * 8;
    PF_HIP(h, h->d_wtA.reserve(need_a, need_a + need_a / 8, Wait::device()));
    PF_HIP(h, hipMemsetAsync(h->d_wtA.get(), 0, h->d_wtA.capacity(), s));
    w.A_h = h->d_wtA.as<long long>();
    w.A_v = reinterpret_cast<long long*>(h->d_wtA.as<char>() + a_bytes);
    h->t_ws_ready = false;                       // (the specialised leg's carve owns the same loss-buffer fields)
    h->wt_ready = true;
    return PF_OK;
}


// dropout and parameter view of one training step of the width-generic leg
static void wide_train_common(pf_handle* h, float dropout_p, uint32_t seed) {
    WtCommon& wc = h->wt_common;
    wc = WtCommon{};
    wc.W = h->d_flat; wc.gpart = h->wt.gpart; wc.gstride = (int)grad_stride(h);
    wc.S = h->cfg.n_hidden_scalars; wc.V = h->cfg.vector_size; wc.N = h->N;
    wc.drop_thr = drop_threshold(dropout_p);
    wc.drop_scale = 1.0f / (1.0f - dropout_p);
    wc.seed = seed;
    wc.mask_override = h->t_mask_override;
}

// What pf_train_forward and the loss entries do once their own arguments are checked: the dropout range, the workspace of the
// selected leg, and the parameters every kernel of this step shares (h->t_common; the wide leg's h->wt_common).  who: the entry
static int train_begin(pf_handle* h, float dropout_p, uint32_t seed, hipStream_t s, const char* who) {
    if (!dropout_ok(dropout_p)) PF_FAIL(h, PF_ERR_ARG, "%s: dropout must be in [0, 1)", who);
    const int rc = h->train_wide ? ensure_wide_train_ws(h, s) : ensure_train_ws(h, s);
    if (rc) return rc;
    if (h->train_wide) wide_train_common(h, dropout_p, seed);
    TrainCommon& tc = h->t_common;
    tc = TrainCommon{};
    tc.W = h->d_flat; tc.gpart = h->t_gpart; tc.nparams = (int)h->nparams; tc.gstride = (int)grad_stride(h);
    tc.tseg = h->d_tseg; tc.ntens = h->n_tseg;
    tc.gpart_enc = h->t_gpart_enc; tc.enc_begin = h->enc_begin; tc.enc_n = h->enc_n;
    tc.drop_thr = drop_threshold(dropout_p); tc.drop_scale = 1.0f / (1.0f - dropout_p); tc.seed = seed;
    tc.mask_override = h->t_mask_override; tc.mask_N = h->N;
    tc.bf16 = h->train_bf16 ? 1 : 0;
    h->t_have_loss = false;                      // a new forward: the unit gradients of an earlier loss are void
    return PF_OK;
}

// every training entry: the specialised gradient path serves 128 / 16 only; other widths need the width-generic leg
#define PF_TRAIN_WIDTH_GUARD(h, who)                                                                                              \
    if ((h) && !(h)->spec && !(h)->train_wide)                                                                                    \
        PF_FAIL(h, PF_ERR_ARG, "%s: training is specialised to n_hidden_scalars 128 / vector_size 16 (this handle: %d / %d; "     \
                               "pf_train_set_family(PF_TRAIN_FAMILY_WIDE) selects the width-generic training leg)", who,          \
                (h)->cfg.n_hidden_scalars, (h)->cfg.vector_size)

int pf_param_count(pf_handle* h, int64_t* n_params, int32_t* n_tensors) {
    int rc = check_ready(h, false);
    if (rc) return rc;
    if (n_params) *n_params = (int64_t)h->nparams;
    if (n_tensors) *n_tensors = (int32_t)h->flat_layout.size();
    return PF_OK;
}

int pf_param_layout(pf_handle* h, int32_t index, const char** name, int64_t* offset, int64_t* numel) {
    int rc = check_ready(h, false);
    if (rc) return rc;
    if (index < 0 || index >= (int32_t)h->flat_layout.size()) PF_FAIL(h, PF_ERR_ARG, "pf_param_layout: index out of range");
    const auto& kv = h->flat_layout[index];
    if (name) *name = kv.first.c_str();
    if (offset) *offset = (int64_t)kv.second.first;
    if (numel) *numel = (int64_t)kv.second.second;
    return PF_OK;
}

// copied: h->d_flat already holds the values (pf_adam_step's kernel wrote them)
static int set_flat_params_impl(pf_handle* h, const float* dev_flat, pf_stream stream, bool copied) {
    int rc = check_ready(h, false);
    if (rc) return rc;
    if (!dev_flat) PF_FAIL(h, PF_ERR_ARG, "pf_set_flat_params: null argument");
    if (!h->d_map) PF_FAIL(h, PF_ERR_STATE, "pf_set_flat_params: no gather map (more than 2^24 parameters)");
    hipStream_t s = (hipStream_t)stream;
    if (!copied) PF_HIP(h, hipMemcpyAsync(h->d_flat, dev_flat, h->nparams * sizeof(float), hipMemcpyDeviceToDevice, s));
    const size_t n_now = (h->pk.n16_begin > 0 && h->pk.n16_begin < h->n_packed) ? h->pk.n16_begin : h->n_packed;
    pfk_gather_weights(h->d_flat, h->d_map, n_now, h->d_w, s);
    h->n16_stale = n_now < h->n_packed;
    ++h->w_version;
    h->t_have_fwd = false;
    return PF_OK;
}

int pf_set_flat_params(pf_handle* h, const float* dev_flat, pf_stream stream) { return set_flat_params_impl(h, dev_flat, stream, false); }

int pf_adam_step(pf_handle* h, float* dev_params, const float* dev_grad, float* dev_exp_avg, float* dev_exp_avg_sq,
                 int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay, pf_stream stream) {
    int rc = check_ready(h, false);
    if (rc) return rc;
    if (!dev_params || !dev_grad || !dev_exp_avg || !dev_exp_avg_sq || step < 1) PF_FAIL(h, PF_ERR_ARG, "pf_adam_step: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
    const bool mirror = h->d_map != nullptr && dev_params != h->d_flat;
    pfk_adam(dev_params, dev_grad, dev_exp_avg, dev_exp_avg_sq, h->nparams, lr, beta1, beta2, eps, weight_decay, (float)bc1,
             (float)std::sqrt(bc2), mirror ? h->d_flat : nullptr, s);
    return set_flat_params_impl(h, dev_params, stream, mirror);
}

// the guarded step's options, checked before anything is enqueued
static int optim_check(pf_handle* h, const char* who, const void* p, const void* g, const void* m, const void* v, const void* state,
                       const pf_optim_opts* o) {
    if (!p || !g || !m || !v || !state || !o) PF_FAIL(h, PF_ERR_ARG, "%s: null argument", who);
    if (reinterpret_cast<uintptr_t>(state) & 7) PF_FAIL(h, PF_ERR_ARG, "%s: the state block must be 8-byte aligned", who);
    for (float x : {o->lr, o->beta1, o->beta2, o->eps, o->weight_decay, o->grad_scale, o->clip, o->ema_decay})
        if (!std::isfinite(x)) PF_FAIL(h, PF_ERR_ARG, "%s: non-finite option", who);
    if (o->beta1 < 0.f || o->beta1 >= 1.f || o->beta2 < 0.f || o->beta2 >= 1.f) PF_FAIL(h, PF_ERR_ARG, "%s: betas must be in [0, 1)", who);
    if (!(o->grad_scale > 0.f)) PF_FAIL(h, PF_ERR_ARG, "%s: grad_scale must be > 0", who);
    if (o->clip < 0.f) PF_FAIL(h, PF_ERR_ARG, "%s: clip must be >= 0", who);
    if (o->ema_decay < 0.f || o->ema_decay >= 1.f) PF_FAIL(h, PF_ERR_ARG, "%s: ema_decay must be in [0, 1)", who);
    if (o->clip_mode != PF_CLIP_NONE && o->clip_mode != PF_CLIP_NORM && o->clip_mode != PF_CLIP_VALUE)
        PF_FAIL(h, PF_ERR_ARG, "%s: unknown clip_mode %d", who, (int)o->clip_mode);
    return PF_OK;
}

// norm, finalising launch and guarded Adam on vectors of length n (pf_optim.hip)
static int optim_launch(pf_handle* h, size_t n, float* p, const float* g, float* m, float* v, float* ema, float* mirror, void* state,
                        const pf_optim_opts* o, hipStream_t s) {
    const size_t n_part = (n + PFO_CHUNK - 1) / PFO_CHUNK;
    PF_HIP(h, h->d_optim_part.reserve(n_part * sizeof(double), n_part * sizeof(double), Wait::none()));
    OptimParams P{};
    P.p = p; P.g = g; P.m = m; P.v = v; P.ema = ema; P.mirror = mirror; P.n = n;
    P.lr = o->lr; P.b1 = o->beta1; P.b2 = o->beta2; P.eps = o->eps; P.wd = o->weight_decay; P.grad_scale = o->grad_scale;
    P.clip_mode = o->clip_mode; P.clip = o->clip; P.ema_decay = o->ema_decay;
    P.partials = h->d_optim_part; P.state = (OptimState*)state;
    pfk_optim_step(P, s);
    return PF_OK;
}

int pf_optim_state_init(pf_handle* h, void* dev_state, int64_t applied_steps, pf_stream stream) {
    if (!h) return PF_ERR_ARG;
    if (!dev_state || (reinterpret_cast<uintptr_t>(dev_state) & 7) || applied_steps < 0)
        PF_FAIL(h, PF_ERR_ARG, "pf_optim_state_init: bad argument");
    pfk_optim_state_init((OptimState*)dev_state, (long long)applied_steps, (hipStream_t)stream);
    return PF_OK;
}

int pf_adam_step_guarded(pf_handle* h, float* dev_params, const float* dev_grad, float* dev_exp_avg, float* dev_exp_avg_sq,
                         float* dev_ema, void* dev_state, const pf_optim_opts* opts, pf_stream stream) {
    int rc = check_ready(h, false);
    if (rc) return rc;
    if ((rc = optim_check(h, "pf_adam_step_guarded", dev_params, dev_grad, dev_exp_avg, dev_exp_avg_sq, dev_state, opts)) != PF_OK) return rc;
    const bool mirror = h->d_map != nullptr && dev_params != h->d_flat;
    if ((rc = optim_launch(h, h->nparams, dev_params, dev_grad, dev_exp_avg, dev_exp_avg_sq, dev_ema, mirror ? h->d_flat : nullptr,
                           dev_state, opts, (hipStream_t)stream)) != PF_OK) return rc;
    return set_flat_params_impl(h, dev_params, stream, mirror);          // (a skipped step re-gathers the unchanged values)
}

int pf_debug_optim_step(pf_handle* h, int64_t n, float* dev_params, const float* dev_grad, float* dev_exp_avg,
                        float* dev_exp_avg_sq, float* dev_ema, void* dev_state, const pf_optim_opts* opts, pf_stream stream) {
    if (!h) return PF_ERR_ARG;
    int rc = optim_check(h, "pf_debug_optim_step", dev_params, dev_grad, dev_exp_avg, dev_exp_avg_sq, dev_state, opts);
    if (rc) return rc;
    if (n < 1) PF_FAIL(h, PF_ERR_ARG, "pf_debug_optim_step: n must be >= 1");
    return optim_launch(h, (size_t)n, dev_params, dev_grad, dev_exp_avg, dev_exp_avg_sq, dev_ema, nullptr, dev_state, opts, (hipStream_t)stream);
}

int pf_debug_optim_chunk(void) { return PFO_CHUNK; }

int pf_get_flat_params(pf_handle* h, float* dev_flat, pf_stream stream) {
    int rc = check_ready(h, false);
    if (rc) return rc;
    if (!dev_flat) PF_FAIL(h, PF_ERR_ARG, "pf_get_flat_params: null argument");
    PF_HIP(h, hipMemcpyAsync(dev_flat, h->d_flat, h->nparams * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PF_OK;
}

int pf_train_forward(pf_handle* h, const float* dev_prot_x, const float* dev_pharm_x, const float* dev_pharm_h,
                     const float* dev_t, float dropout_p, uint32_t seed, float* dev_eps_h, float* dev_eps_x, pf_stream stream) {
    PF_TRAIN_WIDTH_GUARD(h, __func__);
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!dev_pharm_x || !dev_pharm_h || !dev_t || !dev_eps_h || !dev_eps_x) PF_FAIL(h, PF_ERR_ARG, "pf_train_forward: null argument");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = train_begin(h, dropout_p, seed, s, __func__)) != PF_OK) return rc;
    load_state(h, dev_prot_x, dev_pharm_x, dev_pharm_h, s);
    pfk_copy(dev_t, h->d_t, (size_t)h->B, s);
    rc = run_dynamics(h, dev_eps_h, dev_eps_x, s, nullptr, true);
    h->t_have_fwd = rc == PF_OK;
    return rc;
}

// who: the entry the caller used, for the messages (pf_train_loss_forward is the (0, 0) call of pf_train_loss_forward_ep)
static int loss_forward(pf_handle* h, const float* dev_pharm_x0, const float* dev_pharm_h0, const int32_t* dev_t_int,
                        const float* dev_eps_x, const float* dev_eps_h, const float* dev_alpha, const float* dev_sigma,
                        int32_t n_timesteps, float feat_norm, int32_t remove_com, int32_t weighted_loss, int32_t endpoint_param_coord,
                        int32_t endpoint_param_feat, float dropout_p, uint32_t seed, float* dev_out, pf_stream stream, const char* who) {
    PF_TRAIN_WIDTH_GUARD(h, who);
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!dev_pharm_x0 || !dev_pharm_h0 || !dev_t_int || !dev_eps_x || !dev_eps_h || !dev_alpha || !dev_sigma || !dev_out)
        PF_FAIL(h, PF_ERR_ARG, "%s: null argument", who);
    if (n_timesteps < 1 || !(feat_norm > 0.f)) PF_FAIL(h, PF_ERR_ARG, "%s: bad n_timesteps / feat_norm", who);
    // (a dropout_p out of range is reported first, by train_begin: the order of the entry's checks)
    if (dropout_ok(dropout_p) && h->Nf == 0) PF_FAIL(h, PF_ERR_ARG, "%s: the batch has no pharmacophore centers (the losses are means over them)", who);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = train_begin(h, dropout_p, seed, s, who)) != PF_OK) return rc;
    LossParams lp{};
    lp.part = h->d_lpart + 16; lp.ticket = reinterpret_cast<int*>(h->d_lpart);
    lp.B = h->B; lp.Np = h->Np; lp.Nf = h->Nf; lp.nf = h->cfg.pharm_nf; lp.T = n_timesteps; lp.remove_com = remove_com; lp.weighted = weighted_loss;
    lp.feat_norm = feat_norm;
    lp.prot_ptr = h->d_prot_ptr; lp.pharm_ptr = h->d_pharm_ptr; lp.gid = h->d_gid; lp.prot_x0 = h->d_prot_x0;
    lp.x0 = dev_pharm_x0; lp.h0 = dev_pharm_h0; lp.t_int = dev_t_int; lp.eps_x = dev_eps_x; lp.eps_h = dev_eps_h;
    lp.alpha_tab = dev_alpha; lp.sigma_tab = dev_sigma;
    lp.xn = h->d_xn; lp.pharm_h = h->d_pharm_h; lp.t = h->d_t;
    lp.x0c = h->t_lx0c; lp.alpha_g = h->t_lag; lp.sigma_g = h->t_lsg; lp.com2 = h->t_lcom2;
    lp.dyn_h = h->d_eps_h; lp.dyn_x = h->d_eps_x; lp.g_x = h->t_lgx; lp.g_h = h->t_lgh; lp.out = dev_out;
    h->edges_built = false; h->rec_valid = false;
    h->coords_custom = true;                     // the pocket moved with the centers' COM: trajectory constants of the bound coordinates do not apply
    pfk_loss_prepare(&lp, s);
    rc = run_dynamics(h, h->d_eps_h, h->d_eps_x, s, nullptr, true);
    h->t_have_fwd = rc == PF_OK;
    if (rc) return rc;
    pfk_loss_eval(&lp, endpoint_param_coord != 0, endpoint_param_feat != 0, s);
    h->t_have_loss = true;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return PF_OK;
}

int pf_train_loss_forward(pf_handle* h, const float* dev_pharm_x0, const float* dev_pharm_h0, const int32_t* dev_t_int,
                          const float* dev_eps_x, const float* dev_eps_h, const float* dev_alpha, const float* dev_sigma,
                          int32_t n_timesteps, float feat_norm, int32_t remove_com, int32_t weighted_loss, float dropout_p,
                          uint32_t seed, float* dev_out, pf_stream stream) {
    return loss_forward(h, dev_pharm_x0, dev_pharm_h0, dev_t_int, dev_eps_x, dev_eps_h, dev_alpha, dev_sigma, n_timesteps, feat_norm,
                        remove_com, weighted_loss, 0, 0, dropout_p, seed, dev_out, stream, __func__);
}

int pf_train_loss_forward_ep(pf_handle* h, const float* dev_pharm_x0, const float* dev_pharm_h0, const int32_t* dev_t_int,
                             const float* dev_eps_x, const float* dev_eps_h, const float* dev_alpha, const float* dev_sigma,
                             int32_t n_timesteps, float feat_norm, int32_t remove_com, int32_t weighted_loss,
                             int32_t endpoint_param_coord, int32_t endpoint_param_feat, float dropout_p, uint32_t seed,
                             float* dev_out, pf_stream stream) {
    return loss_forward(h, dev_pharm_x0, dev_pharm_h0, dev_t_int, dev_eps_x, dev_eps_h, dev_alpha, dev_sigma, n_timesteps, feat_norm,
                        remove_com, weighted_loss, endpoint_param_coord, endpoint_param_feat, dropout_p, seed, dev_out, stream, __func__);
}

static int loss_backward(pf_handle* h, const float* g_pos, const float* g_pos2, const float* g_feat, const float* g_feat2,
                         float* dev_grad, pf_stream stream, const char* who) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!h->t_have_fwd || !h->t_have_loss) PF_FAIL(h, PF_ERR_STATE, "%s: no pf_train_loss_forward on this batch", who);
    if (!g_pos || !g_feat || !dev_grad) PF_FAIL(h, PF_ERR_ARG, "%s: null argument", who);
    // the unit gradients times their upstream scalars: as extra blocks of the backward's first launch (the fragment re-pack) when it
    // has one, else as a launch of its own (pf_train_backward)
    h->pend_scale = ScaleArgs{h->t_lgx, h->Nf * 3, g_pos, g_pos2, h->t_lgh, h->Nf * h->cfg.pharm_nf, g_feat, g_feat2};
    h->has_pend_scale = true;
    h->t_have_loss = false;                      // the unit gradients are consumed
    rc = pf_train_backward(h, h->t_lgh, h->t_lgx, dev_grad, stream);
    h->has_pend_scale = false;
    return rc;
}

int pf_train_loss_backward(pf_handle* h, const float* dev_g_pos, const float* dev_g_feat, float* dev_grad, pf_stream stream) {
    PF_TRAIN_WIDTH_GUARD(h, __func__);
    return loss_backward(h, dev_g_pos, nullptr, dev_g_feat, nullptr, dev_grad, stream, "pf_train_loss_backward");
}

int pf_train_loss_backward_out(pf_handle* h, const float* dev_g_out, float* dev_grad, pf_stream stream) {
    PF_TRAIN_WIDTH_GUARD(h, __func__);
    if (h && !dev_g_out) PF_FAIL(h, PF_ERR_ARG, "pf_train_loss_backward_out: null argument");
    // upstream gradients of the nine outputs: [0] and [1] of the two losses, [6] of their sum; the metrics carry none
    return loss_backward(h, dev_g_out, dev_g_out ? dev_g_out + 6 : nullptr, dev_g_out ? dev_g_out + 1 : nullptr,
                         dev_g_out ? dev_g_out + 6 : nullptr, dev_grad, stream, "pf_train_loss_backward_out");
}


// ---- the backward pass of the width-generic leg: the reverse of run_dynamics_wide (pf_wide_train.hip lists the launches) ----
// One level of a chain (the message chains of a conv layer, its update chains, the noise head): the GVP table and level, the
// level's input rows (already at the level) and buf_s / buf_v as upstream and output gradient alike, all rows of one shape.
// The caller's: the tile table, sv_base, the head's output of level 0, what only the message chains read
static WtChainParams wt_chain_params(const pf_handle* h, const GvpT* g, int g_stride, int n_levels, int lv, const float* sv_s,
                                     const float* sv_v, float* buf_s, float* buf_v, int ls, int lvw) {
    WtChainParams q{};
    q.c = h->wt_common; q.dyn_cnt = h->d_dyn_cnt;
    q.g = g; q.g_stride = g_stride; q.level = lv; q.last = lv == n_levels - 1;
    q.sv_s = sv_s; q.sv_v = sv_v; q.sv_ls = ls; q.sv_lv = lvw;
    q.up_s = buf_s; q.up_v = buf_v; q.up_ls = ls; q.up_lv = lvw;
    q.out_s = buf_s; q.out_v = buf_v; q.out_ls = ls; q.out_lv = lvw;
    return q;
}
// One of conv layer l's two GVPLayerNorms with the GVPDropout next to it (which: 0 message_layer_norms, 1 update_layer_norms):
// tiles, the rows the forward normalised, the norm's parameters, the dropout stream.  The caller's: dyA / dyB, out1 / out2
static WtNormParams wt_norm_params(const pf_handle* h, const LayerTiles& lt, int l, int which) {
    const pf_config& c = h->cfg;
    const size_t row0 = (size_t)l * h->N, S = c.n_hidden_scalars, V3 = (size_t)3 * c.vector_size;
    WtNormParams n{};
    n.c = h->wt_common; n.tiles = lt.ntiles; n.n_tiles = lt.n_ntiles; n.dyn_cnt = h->d_dyn_cnt; n.row_ids = h->d_act_ids;
    n.gid = h->d_gid; n.gnorm = h->d_gnorm; n.B = h->B; n.norm_mode = c.message_norm_mode; n.norm_value = c.message_norm_value;
    for (int nt = 0; nt < 2; ++nt) {
        const int* o = &h->po.ln[(size_t)(l * 2 + nt) * 4 + 2 * which];
        n.o_lw[nt] = o[0]; n.o_lb[nt] = o[1];
    }
    n.x_s = (which ? h->wt.x2_s : h->wt.x1_s) + row0 * S; n.x_v = (which ? h->wt.x2_v : h->wt.x1_v) + row0 * V3;
    n.stream = l * 2 + which; n.use_norm = which ? 0 : 1;
    return n;
}
// the centers' sums of the per-edge dL/d(x_src - x_dst) rows of every conv layer (g_diff [n_convs][layer_stride][3]: the wide leg's
// or the tuned family's -- the kernel reads the edge-slot layout the two share)
static WtCenterSumParams wt_center_sum_params(const pf_handle* h, const float* g_diff, size_t layer_stride, float* g_x) {
    WtCenterSumParams p{};
    p.Np = h->Np; p.Nf = h->Nf; p.N = h->N; p.B = h->B; p.L = h->cfg.n_convs;
    p.g_diff = g_diff; p.layer_stride = layer_stride;
    p.in_start = h->d_in_start; p.in_cnt = h->d_in_cnt; p.reg = h->d_reg; p.dyn_cnt = h->d_dyn_cnt;
    p.esrc = h->d_esrc; p.gid = h->d_gid; p.g_x = g_x;
    return p;
}
// g_x / g_h: dL/d(center coordinates) [Nf][3] / dL/d(center feature rows) [Nf][pharm_nf] of the same scalar, or NULL -- with both
// NULL the launches and every bit of the parameter gradient are those of the plain backward.
// dev_grad == NULL: the inputs-only pass (pf_dynamics_input_vjp, a guided step).  The gradient copies are neither cleared nor summed,
// every kernel runs in its form without weight-gradient products, and the encoders' backward runs only for g_h (its center tiles).
// The per-row gradients take the same operations in both forms: g_x and g_h are the full pass's bits
static int wide_train_backward(pf_handle* h, const float* g_eps_h, const float* g_eps_x, float* dev_grad, float* g_x, float* g_h,
                               hipStream_t s) {
    const bool full = dev_grad != nullptr;
    const int wg = (full || h->vjp_full_kernels) ? 1 : 0;      // the kernels' form (PFDYN_VJP_FULL_KERNELS: sums into copies nobody reads)
    const pf_config& c = h->cfg;
    const int L = c.n_convs, N = h->N, S = c.n_hidden_scalars, V = c.vector_size, V3 = 3 * V, ES = S + PF_R, EV = V3 + 3;
    const int nm = c.n_message_gvps, nu = c.n_update_gvps, nh = c.n_noise_gvps;
    pf_handle::WtWs& w = h->wt;
    const WtCommon& wc = h->wt_common;
    if (h->has_pend_scale) {
        const ScaleArgs& a = h->pend_scale;
        pfk_scale_loss(a.gx, a.nx, a.a, a.a2, a.gh, a.nh, a.b, a.b2, s);
        h->has_pend_scale = false;
    }
    if (full) PF_HIP(h, hipMemsetAsync(w.gpart, 0, (size_t)PFWT_NB * wc.gstride * sizeof(float), s));
    PF_HIP(h, hipMemsetAsync(h->d_wtA.get(), 0, h->d_wtA.capacity(), s));
    pfk_fix_scale(g_eps_h, h->Nf * c.pharm_nf, g_eps_x, h->Nf * 3, w.fix, s);
    // (a layer's level-0 launch stores the rows of the slots it walks; the others -- the last layer's fp slots -- stay zero)
    if (g_x) PF_HIP(h, hipMemsetAsync(w.gdiff, 0, (size_t)L * w.Es * 3 * sizeof(float), s));
    int a = 0;
    {   // head: to_scalar_output, then its levels; the first level's input gradient is dL/d(last layer output) of the centers
        WtHeadOutParams p{};
        p.c = wc; p.Np = h->Np; p.Nf = h->Nf; p.pharm_nf = c.pharm_nf; p.g_eps_h = g_eps_h; p.g_eps_x = g_eps_x; p.h64 = w.h64;
        p.o_Wout = h->po.out_w; p.o_bout = h->po.out_b;
        p.up_s = w.gch_s; p.up_v = w.gch_v; p.up_ls = S; p.up_lv = V3;
        pfk_wt_head_out(&p, wg, s);
        const size_t Nf1 = (size_t)std::max(h->Nf, 1);
        for (int lv = nh - 1; lv >= 0; --lv) {
            WtChainParams q = wt_chain_params(h, h->d_gvpt + h->head_base(), 0, nh, lv, w.hsv_s + (size_t)lv * Nf1 * S,
                                              w.hsv_v + (size_t)lv * Nf1 * V3, w.gch_s, w.gch_v, S, V3);
            q.ntiles = h->d_node_tiles; q.n_tiles = h->n_node_tiles_last; q.row_ids = h->d_act_ids; q.sv_base = h->Np;
            if (lv == 0) { q.out_s = w.G_s[a]; q.out_v = w.G_v[a]; }
            ProfScope ps(h, pf_handle::K_BWD_HEAD, s);
            pfk_wt_chain(&q, 0, wg, s);
        }
    }
    for (int l = L - 1; l >= 0; --l) {
        const LayerTiles lt = layer_tiles(h, l);    // the forward's tile lists: rows it did not compute have no backward
        PF_HIP(h, hipMemsetAsync(w.G_s[a ^ 1], 0, (size_t)N * S * sizeof(float), s));
        PF_HIP(h, hipMemsetAsync(w.G_v[a ^ 1], 0, (size_t)N * V3 * sizeof(float), s));
        {   // LayerNorm 2 and the residual dropout
            WtNormParams n = wt_norm_params(h, lt, l, 1);
            n.dyA_s = w.G_s[a]; n.dyA_v = w.G_v[a];
            n.out1_s = w.gres_s; n.out1_v = w.gres_v; n.out2_s = w.gch_s; n.out2_v = w.gch_v;
            ProfScope ps(h, pf_handle::K_BWD_NODE, s);
            pfk_wt_norm(&n, wg, s);
        }
        for (int lv = nu - 1; lv >= 0; --lv) {
            const size_t row0 = ((size_t)l * nu + lv) * N;
            WtChainParams q = wt_chain_params(h, h->d_gvpt + h->upd_base(l, 0), nu, nu, lv, w.usv_s + row0 * S, w.usv_v + row0 * V3,
                                              w.gch_s, w.gch_v, S, V3);
            q.ntiles = lt.ntiles; q.n_tiles = lt.n_ntiles; q.row_ids = h->d_act_ids;
            ProfScope ps(h, pf_handle::K_BWD_NODE, s);
            pfk_wt_chain(&q, 0, wg, s);
        }
        {   // the residual joins, LayerNorm 1, the message dropout and norm: dL/d(layer input) (residual path), dL/d(aggregate)
            WtNormParams n = wt_norm_params(h, lt, l, 0);
            n.dyA_s = w.gch_s; n.dyA_v = w.gch_v; n.dyB_s = w.gres_s; n.dyB_v = w.gres_v;
            n.out1_s = w.G_s[a ^ 1]; n.out1_v = w.G_v[a ^ 1]; n.out2_s = w.gagg_s; n.out2_v = w.gagg_v;
            ProfScope ps(h, pf_handle::K_BWD_NODE, s);
            pfk_wt_norm(&n, wg, s);
        }
        for (int lv = nm - 1; lv >= 0; --lv) {
            const size_t row0 = ((size_t)l * nm + lv) * w.Es;
            WtChainParams q = wt_chain_params(h, h->d_gvpt + h->msg_base(l, 0), nm, nm, lv, w.esv_s + row0 * ES, w.esv_v + row0 * EV,
                                              w.ges, w.gev, ES, EV);
            q.etiles = lt.etiles; q.n_tiles = lt.n_etiles;
            q.esrc = h->d_esrc; q.edst = h->d_edst; q.gagg_s = w.gagg_s; q.gagg_v = w.gagg_v;
            q.in_cnt = h->d_in_cnt; q.pp_slot = lt.pp_slot; q.norm_mode = c.message_norm_mode; q.l0 = l == 0;
            q.A_h = w.A_h; q.A_v = w.A_v; q.fix = w.fix;
            if (g_x && lv == 0) {
                q.g_diff = w.gdiff + (size_t)l * w.Es * 3; q.xn = reinterpret_cast<const float4*>(w.xkeep);
                q.rbf_sigma = rbf_params(c, q.rbf_mu, nullptr);
            }
            ProfScope ps(h, pf_handle::K_BWD_EDGE_LEVEL, s);
            pfk_wt_chain(&q, 1, wg, s);
        }
        pfk_fix_apply(w.A_h, w.G_s[a ^ 1], (size_t)N * S, w.fix, s);
        if (l != 0) pfk_fix_apply(w.A_v, w.G_v[a ^ 1], (size_t)N * V3, w.fix, s);      // conv layer 0 has no vector input
        a ^= 1;
    }
    if (full || g_h) {
        WtEncParams p{};
        p.c = wc; p.Np = h->Np; p.Nf = h->Nf; p.rec_nf = c.rec_nf; p.pharm_nf = c.pharm_nf;
        p.prot_h0 = h->d_prot_h0; p.pharm_h = h->d_pharm_h; p.t = h->d_t; p.gid = h->d_gid;
        for (int nt = 0; nt < 2; ++nt) { p.o_w[nt] = h->po.enc[nt][0]; p.o_b[nt] = h->po.enc[nt][1]; p.o_lw[nt] = h->po.enc[nt][2]; p.o_lb[nt] = h->po.enc[nt][3]; }
        p.G_h = w.G_s[a]; p.g_pharm_h = g_h;
        pfk_wt_encode(&p, wg, s);
    }
    if (g_x) {
        const WtCenterSumParams p = wt_center_sum_params(h, w.gdiff, w.Es, g_x);
        pfk_wt_center_sum(&p, s);
    }
    if (full) pfk_wt_reduce(w.gpart, wc.gstride, dev_grad, (int)h->nparams, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return PF_OK;
}

// ---- the backward pass of the specialised gradient kernels: a sequencer like run_dynamics --------------------------------------
// What one pf_train_backward call computes once and its pieces share (a plain struct on the entry's stack).  The rule: a piece is
// named for what it launches, every parameter struct has one builder, and which tiles a layer walks is layer_tiles' to say.
struct BwdCall {
    pf_handle* h; hipStream_t s; const float *g_eps_h, *g_eps_x;
    // pf_train_set_input_grads: dL/d(center coordinates) [Nf][3], dL/d(center feature rows) [Nf][pharm_nf], or NULL.  full: the pass
    // has a parameter gradient to give (false: pf_dynamics_input_vjp and the guided step -- no reduce, early or final, and the
    // encoders' backward only for g_h, on its center tiles)
    float *g_x, *g_h; bool full;
    hipStream_t side; bool side_on;         // the handle's side stream; it is another stream than the caller's (always, unless the caller passes it)
    TrainCommon tc;                         // h->t_common with this call's k_pack_gvp tables
    ReduceParams rp;                        // the final reduce; the early one is a copy with its own class mask
    int a;                                  // t_G_*[a]: dL/d(output) of the layer being differentiated, [a ^ 1]: dL/d(its input)
    bool first_clear_done;                  // the side stream cleared the last layer's input gradients
    bool enc_grouped_done;                  // conv layer 0's join grouped the protein rows for the encoders (k_fix_enc_group)
    unsigned early_mask;                    // classes the early reduce summed
};
static int bwd_grid(int nb, int ntiles) { return ntiles > 0 ? std::max(1, std::min(nb, 2 * ntiles)) : 0; }
// edge slots per conv layer in d_gdiff
static size_t gdiff_layer_stride(const pf_handle* h) { return (size_t)std::max<int64_t>(h->Ecap, 1); }
// (the encoders' backward differentiates the protein rows grouped by (graph, element) when the features can be one-hots)
static bool enc_grouped(const pf_handle* h) { return h->cfg.rec_nf <= 16 && h->Np > 0; }
// which gradient copies hold what: the grid of every launch of the pass, known before the first one
static ReduceParams reduce_params(const pf_handle* h, float* dev_grad) {
    ReduceParams rp{};
    rp.gpart = h->t_gpart; rp.nparams = (int)h->nparams; rp.gstride = (int)grad_stride(h); rp.grad = dev_grad;
    rp.tseg = h->d_tseg; rp.ntens = h->n_tseg; rp.NB = h->t_nblk; rp.ccnt = h->t_ccnt;
    rp.gpart_enc = h->t_gpart_enc; rp.enc_begin = h->enc_begin; rp.enc_n = h->enc_n;
    rp.head_grid = bwd_grid(h->t_nblk, h->n_head_tiles);
    for (int l = 0; l < h->cfg.n_convs; ++l) {
        const LayerTiles lt = layer_tiles(h, l);
        rp.node_grid[l] = bwd_grid(h->t_nblk, lt.n_ntiles); rp.n_et[l] = lt.n_et;
    }
    rp.enc_grid = std::max(1, std::min(PFT_ENC_BLOCKS, (h->Np + PFT_ROWS - 1) / PFT_ROWS + (h->Nf + PFT_ROWS - 1) / PFT_ROWS));
    return rp;
}
// the fragment tables of k_bwd_edge_level (re-packed when the weights moved), the loss's unit gradients times their upstream
// scalars (extra blocks of the re-pack when there is one, else a launch of their own), the accumulators an aborted pass left dirty
static int bwd_prologue(BwdCall& bc, float* dev_grad) {
    pf_handle* h = bc.h;
    const bool scale_now = h->has_pend_scale;
    h->has_pend_scale = false;
    if (h->wpack_version != h->w_version) {
        const int ng = h->n_gvpt;
        const size_t wpack_bytes = (size_t)2 * std::max(ng, 1) * PFT_WPACK_FLOATS * sizeof(float);       // (released by every commit)
        PF_HIP(h, h->d_wpack.reserve(wpack_bytes, wpack_bytes, Wait::none()));
        pfk_pack_gvp(h->d_flat, h->d_gvpt, ng, h->d_wpack, h->d_wpack + (size_t)ng * PFT_WPACK_FLOATS, scale_now ? &h->pend_scale : nullptr, bc.s);
        h->wpack_version = h->w_version;
    } else if (scale_now) {
        const ScaleArgs& a = h->pend_scale;
        pfk_scale_loss(a.gx, a.nx, a.a, a.a2, a.gh, a.nh, a.b, a.b2, bc.s);
    }
    h->t_common.wpack_b = h->d_wpack; h->t_common.wpack_f = h->d_wpack + (size_t)h->n_gvpt * PFT_WPACK_FLOATS;
    bc.tc = h->t_common;
    bc.rp = reduce_params(h, dev_grad);
    if (h->tA_dirty) PF_HIP(h, hipMemsetAsync(h->d_tA.get(), 0, h->d_tA.capacity(), bc.s));      // an earlier pass stopped half way
    h->tA_dirty = true;
    return PF_OK;
}
// the dense work lists of conv layer l (k_compact_node_rows, k_compact_rows: one or two workgroups each, 10-20 us)
static void bwd_work_lists(BwdCall& bc, int l, hipStream_t on) {
    pf_handle* h = bc.h;
    const LayerTiles lt = layer_tiles(h, l);
    pfk_compact_node_rows(lt.ntiles, lt.n_ntiles, h->d_dyn_cnt, h->d_act_ids, h->N, h->t_ulist + h->t_ulist_cap * l, h->t_ucap, h->t_ccnt + 96 + 4 * l, on);
    pfk_compact_rows(lt.etiles, lt.et_tile0, lt.n_et, h->d_dyn_cnt, h->t_clist + h->t_clist_cap * l, h->t_ccnt + 16 * l, on);
}
// The per-edge dL/d(x_src - x_dst) rows of all conv layers: a level-0 launch stores the rows of the slots it walks, the others (the
// last layer's fp slots, slots past a region's live count) must read as zeros in the centers' sums.  Cleared once per pass, in the
// batch that clears the last layer's input gradients
static void bwd_add_gdiff_clear(const BwdCall& bc, ZeroBatch& zb) {
    const pf_handle* h = bc.h;
    if (bc.g_x) zb.add(h->d_gdiff.get(), (size_t)h->cfg.n_convs * gdiff_layer_stride(h) * 3 * sizeof(float));
}
// The work lists depend on the forward's edge counts only: they are built on the side stream while the head's backward runs on
// the caller's.  Two groups: what the first layer of the loop needs at once (its work lists, its cleared input gradients: cmp_ev[1]),
// then the rest (the fixed-point scale, first read by that layer's edge kernels; the other layers' lists: cmp_ev[2], waited for
// behind that layer's node kernel) -- as one group the side stream outlasted the head's backward by 28 us once that took 59
static int bwd_side_lists(BwdCall& bc) {
    pf_handle* h = bc.h;
    const int L = h->cfg.n_convs;
    PF_HIP(h, h->s_side.get(&bc.side));
    hipStream_t side = bc.side;
    bc.side_on = side != bc.s;
    if (bc.side_on) { PF_HIP(h, h->cmp_ev[0].record(bc.s)); PF_HIP(h, h->cmp_ev[0].hold(side)); }
    bwd_work_lists(bc, L - 1, side);
    if (bc.side_on) {
        // the first layer of the loop receives its input gradients in G[1]: cleared here, under the head's backward
        ZeroBatch zb(side);
        zb.add(h->t_G_h[1], (size_t)h->N * PF_S * 4);
        if (L - 1 != 0) zb.add(h->t_G_v[1], (size_t)h->N * 48 * 4);
        bwd_add_gdiff_clear(bc, zb);
        zb.flush();
        bc.first_clear_done = true;
        PF_HIP(h, h->cmp_ev[1].record(side));
    }
    pfk_fix_scale(bc.g_eps_h, h->Nf * h->cfg.pharm_nf, bc.g_eps_x, h->Nf * 3, h->t_fix, side);
    for (int l = L - 2; l >= 0; --l) bwd_work_lists(bc, l, side);
    if (bc.side_on) PF_HIP(h, h->cmp_ev[2].record(side));
    return PF_OK;
}
// (the head kernel stores dL/d(last layer output) for every pharm row, and the last layer's node kernel reads those rows
// only: no clearing of t_G_*[0] in front of it)
static void bwd_head_launch(BwdCall& bc) {
    pf_handle* h = bc.h;
    const pf_config& c = h->cfg;
    BwdHeadParams p{};
    p.c = bc.tc; p.tiles = h->d_head_tiles; p.ntiles = h->n_head_tiles; p.node_base = h->Np;
    p.h = h->t_H[c.n_convs]; p.v = h->t_V[c.n_convs];
    p.g = h->d_gvpt + h->head_base(); p.n_gvps = c.n_noise_gvps;
    p.o_Wout = h->po.out_w; p.o_bout = h->po.out_b;
    p.pharm_nf = c.pharm_nf; p.g_eps_h = bc.g_eps_h; p.g_eps_x = bc.g_eps_x;
    p.G_h = h->t_G_h[0]; p.G_v = h->t_G_v[0];
    if (h->t_head_saved) { p.sv_z = h->t_hsv_z; p.sv_g = h->t_hsv_g; p.sv_v = h->t_hsv_v; p.sv_stride = (size_t)h->Nf; }
    ProfScope ps(h, pf_handle::K_BWD_HEAD, bc.s);
    pfk_bwd_head(&p, bc.rp.head_grid, bc.s);
}
static BwdNodeParams bwd_node_params(const BwdCall& bc, int l) {
    const pf_handle* h = bc.h;
    const pf_config& c = h->cfg;
    const LayerTiles lt = layer_tiles(h, l);
    const int a = bc.a;
    BwdNodeParams n{};
    n.c = bc.tc; n.tiles = lt.ntiles; n.ntiles = lt.n_ntiles;
    n.pp_slot = lt.pp_slot; n.row_ids = h->d_act_ids; n.dyn_cnt = h->d_dyn_cnt;
    n.in_start = h->d_in_start; n.in_cnt = h->d_in_cnt; n.N = h->N;
    n.msg_s = h->t_msg_s[l]; n.msg_v = h->t_msg_v[l]; n.zero_row = h->zero_row;
    n.h_in = h->t_H[l]; n.v_in = h->t_V[l];
    n.G_h_out = h->t_G_h[a]; n.G_v_out = h->t_G_v[a]; n.G_h_in = h->t_G_h[a ^ 1]; n.G_v_in = h->t_G_v[a ^ 1];
    n.gagg_s = h->t_gagg_s; n.gagg_v = h->t_gagg_v;
    n.gid = h->d_gid; n.gnorm = h->d_gnorm; n.B = h->B;
    n.norm_mode = c.message_norm_mode; n.norm_value = c.message_norm_value;
    n.upd = h->d_gvpt + h->upd_base(l, 0); n.n_upd = c.n_update_gvps;
    for (int nt = 0; nt < 2; ++nt)
        for (int k = 0; k < 4; ++k) n.o_ln[nt][k] = h->po.ln[(size_t)(l * 2 + nt) * 4 + k];
    n.layer = l; n.l0 = l == 0;
    n.grp = (int)h->t_grp.size() > l ? h->t_grp[l] : 32;
    if ((int)h->t_node_saved.size() > l && h->t_node_saved[l]) {
        n.sv_z = h->t_nsv_z[l]; n.sv_g = h->t_nsv_g[l]; n.sv_v = h->t_nsv_v[l]; n.sv_stride = (size_t)2 * h->N;
    }
    n.ulist = h->t_ulist + h->t_ulist_cap * l; n.ucnt = h->t_ccnt + 96 + 4 * l; n.ucap = h->t_ucap;
    return n;
}
// The node kernel stores dL/d(layer input) for the rows it walks and the edge kernels add to it: cleared first, unless the side
// stream has (the last layer's)
static void bwd_node_launch(BwdCall& bc, int l) {
    pf_handle* h = bc.h;
    const bool last = l == h->cfg.n_convs - 1;
    if (!(last && bc.first_clear_done)) {
        ZeroBatch zb(bc.s);
        zb.add(h->t_G_h[bc.a ^ 1], (size_t)h->N * PF_S * 4);
        if (l != 0) zb.add(h->t_G_v[bc.a ^ 1], (size_t)h->N * 48 * 4);      // (conv layer 0 has no vector input: nobody writes or reads that gradient)
        if (last) bwd_add_gdiff_clear(bc, zb);
        zb.flush();
    }
    const BwdNodeParams n = bwd_node_params(bc, l);
    ProfScope ps(h, pf_handle::K_BWD_NODE, bc.s);
    pfk_bwd_node(&n, bc.rp.node_grid[l], bc.s);
}
// the message chains of conv layer l; level and fx are set per launch
static BwdEdgeLevelParams bwd_edge_params(const BwdCall& bc, int l) {
    const pf_handle* h = bc.h;
    const pf_config& c = h->cfg;
    const LayerTiles lt = layer_tiles(h, l);
    BwdEdgeLevelParams e{};
    e.c = bc.tc; e.tiles = lt.etiles; e.dyn_cnt = h->d_dyn_cnt;
    e.pp_slot = lt.pp_slot;
    for (int et = 0; et <= 4; ++et) e.et_tile0[et] = lt.et_tile0[et];
    e.n_et = lt.n_et;
    e.clist = h->t_clist + h->t_clist_cap * l; e.ccnt = h->t_ccnt + 16 * l;
    e.esrc = h->d_esrc; e.edst = h->d_edst; e.xn = h->d_xn;
    e.h = h->t_H[l]; e.v = h->t_V[l];
    e.gagg_s = h->t_gagg_s; e.gagg_v = h->t_gagg_v; e.in_cnt = h->d_in_cnt; e.N = h->N;
    e.norm_mode = c.message_norm_mode;
    e.G_h_in = h->t_G_h[bc.a ^ 1]; e.G_v_in = h->t_G_v[bc.a ^ 1];
    e.sv_z = h->t_sv_z[l]; e.sv_g = h->t_sv_g[l]; e.sv_v = h->t_sv_v[l];
    e.sv_stride = (size_t)std::max<int64_t>(h->Ecap, 1);
    e.gs_buf = h->t_gs_buf; e.gv_buf = h->t_gv_buf;
    e.g = h->d_gvpt + h->msg_base(l, 0); e.n_gvps = c.n_message_gvps;
    e.rbf_sigma = rbf_params(c, e.rbf_mu, &e.rbf_inv_sigma);
    e.l0 = l == 0;
    e.A_h = h->t_A_h; e.A_v = h->t_A_v; e.fix = h->t_fix;
    e.wpack = h->d_wpack + (size_t)h->msg_base(l, 0) * PFT_WPACK_FLOATS;
    return e;
}
static void bwd_edge_levels(BwdCall& bc, int l) {
    pf_handle* h = bc.h;
    const int nm = h->cfg.n_message_gvps;
    BwdEdgeLevelParams e = bwd_edge_params(bc, l);
    for (int lv = nm - 1; lv >= 0; --lv) {
        e.level = lv;
        e.fx = h->no_fixed_shapes ? 0 : h->po.edge_fx[(size_t)l * nm + lv];
        // level 0 with dL/d(center coordinates) asked for: the launch with the geometry epilogue, into this layer's rows of d_gdiff
        e.g_diff = (bc.g_x && lv == 0) ? h->d_gdiff.as<float>() + (size_t)l * gdiff_layer_stride(h) * 3 : nullptr;
        ProfScope ps(h, pf_handle::K_BWD_EDGE_LEVEL, bc.s);
        pfk_bwd_edge_level(&e, h->t_nblk, bc.s);
    }
}
// How conv layer l's fixed-point sums (the level-0 scatter to the source nodes) join dL/d(layer input):
//   JOIN_ACTIVE_ROWS  the last layer's ff / pf edges scatter into pharm rows and active protein atoms only: the pruned layout's node tiles
//   JOIN_ENC_GROUP    conv layer 0: in the pass that also groups the protein rows by (graph, element) for the encoders
//   JOIN_ALL_ROWS     every row (and, above conv layer 0, every vector row)
enum FixJoin { JOIN_ACTIVE_ROWS, JOIN_ENC_GROUP, JOIN_ALL_ROWS };
static FixJoin fix_join_form(const pf_handle* h, int l) {
    const bool last = l == h->cfg.n_convs - 1;
    if (last && l != 0 && prune_layer(h) >= 0 && h->d_act_ids != nullptr && h->n_node_tiles_act > 0) return JOIN_ACTIVE_ROWS;
    if (l == 0 && enc_grouped(h) && !h->no_fix_fuse) return JOIN_ENC_GROUP;
    return JOIN_ALL_ROWS;
}
static void bwd_fix_join(BwdCall& bc, int l) {
    pf_handle* h = bc.h;
    float *G_h_in = h->t_G_h[bc.a ^ 1], *G_v_in = h->t_G_v[bc.a ^ 1];
    const FixJoin form = fix_join_form(h, l);
    if (form == JOIN_ACTIVE_ROWS)
        pfk_fix_apply_rows(h->d_node_tiles_act, h->n_node_tiles_act, h->d_dyn_cnt, h->d_act_ids, h->t_A_h, G_h_in, h->t_A_v, G_v_in, h->t_fix, bc.s);
    else if (form == JOIN_ENC_GROUP) {
        pfk_fix_enc_group(h->t_A_h, G_h_in, h->t_fix, h->d_prot_ptr, h->d_ptype, h->B, h->cfg.rec_nf, h->t_Gg, h->Np, h->Nf, h->d_l0flag, bc.s);
        bc.enc_grouped_done = true;
    } else {
        pfk_fix_apply(h->t_A_h, G_h_in, (size_t)h->N * PF_S, h->t_fix, bc.s);
        if (l != 0) pfk_fix_apply(h->t_A_v, G_v_in, (size_t)h->N * 48, h->t_fix, bc.s);      // conv layer 0 has no vector input
    }
}
// The head's and the last layer's node and message classes are complete: with more layers to go, their gradient copies are
// summed on the side stream now (bandwidth-bound, ~140 MB) under the next layer's kernels
static int bwd_early_reduce(BwdCall& bc, int l) {
    pf_handle* h = bc.h;
    ReduceParams early = bc.rp;
    early.cls_mask = (1u << PFT_CLS_HEAD) | (1u << (PFT_CLS_NODE + l));
    for (int et = 0; et < 4; ++et) early.cls_mask |= 1u << (PFT_CLS_MSG + l * 4 + et);
    PF_HIP(h, h->cmp_ev[0].record(bc.s));
    PF_HIP(h, h->cmp_ev[0].hold(bc.side));
    pfk_train_reduce(&early, bc.side);
    PF_HIP(h, h->cmp_ev[1].record(bc.side));
    bc.early_mask = early.cls_mask;
    return PF_OK;
}
static void bwd_encoders(BwdCall& bc) {
    pf_handle* h = bc.h;
    const pf_config& c = h->cfg;
    BwdEncodeParams p{};
    p.c = bc.tc; p.Np = h->Np; p.Nf = h->Nf;
    p.prot_h0 = h->d_prot_h0; p.pharm_h = h->d_pharm_h; p.t = h->d_t; p.gid = h->d_gid;
    p.rec_nf = c.rec_nf; p.pharm_nf = c.pharm_nf;
    for (int nt = 0; nt < 2; ++nt) { p.o_w[nt] = h->po.enc[nt][0]; p.o_b[nt] = h->po.enc[nt][1]; p.o_lw[nt] = h->po.enc[nt][2]; p.o_lb[nt] = h->po.enc[nt][3]; }
    p.G_h = h->t_G_h[bc.a];
    p.B = h->B; p.onehot_flag = h->d_l0flag;
    p.Gg = enc_grouped(h) ? h->t_Gg : nullptr;
    p.g_pharm_h = bc.g_h; p.pharm_only = bc.full ? 0 : 1;
    if (p.Gg && !bc.enc_grouped_done && bc.full) pfk_enc_group(p.G_h, h->d_prot_ptr, h->d_ptype, h->B, c.rec_nf, h->t_Gg, bc.s);
    pfk_bwd_encode(&p, bc.rp.enc_grid, bc.s);
}
// dL/d(center coordinates): the centers' sums of the rows the level-0 launches left in d_gdiff
static void bwd_center_sum(BwdCall& bc) {
    const pf_handle* h = bc.h;
    const WtCenterSumParams p = wt_center_sum_params(h, h->d_gdiff.as<const float>(), gdiff_layer_stride(h), bc.g_x);
    pfk_wt_center_sum(&p, bc.s);
}

// Input gradients on the tuned family (the wide family always has them): the switch, and fp32.  Refused before anything is
// launched: the kept forward stays usable
static int tuned_input_grads_guard(pf_handle* h, const char* who) {
    if (h->train_wide) return PF_OK;
    if (!h->train_in_grads)
        PF_FAIL(h, PF_ERR_ARG, "%s: gradients w.r.t. the center coordinates and features are computed by the width-generic training "
                               "leg only (pf_train_set_family(PF_TRAIN_FAMILY_WIDE), fp32, every supported width)", who);
    if (h->train_bf16)
        PF_FAIL(h, PF_ERR_ARG, "%s: the tuned family's input gradients (pf_train_set_input_grads) are fp32 only: "
                               "pf_train_set_precision(PF_TRAIN_F32) first", who);
    return PF_OK;
}
// The tuned family's backward of the kept forward.  dev_grad == NULL: the inputs-only pass (pf_dynamics_input_vjp, a guided step) --
// the same launches without the reduces (the kernels run in their full form: their weight-gradient products land in gradient
// copies nobody sums) and the encoders' backward only for g_h.  g_x / g_h as in wide_train_backward; with both NULL and a dev_grad
// the launches are the plain backward's
static int tuned_train_backward(pf_handle* h, const float* g_eps_h, const float* g_eps_x, float* dev_grad, float* g_x, float* g_h,
                                hipStream_t s) {
    int rc;
    const int L = h->cfg.n_convs;
    BwdCall bc{};
    bc.h = h; bc.s = s; bc.g_eps_h = g_eps_h; bc.g_eps_x = g_eps_x;
    bc.g_x = g_x; bc.g_h = g_h; bc.full = dev_grad != nullptr;
    if (g_x) {
        const size_t need = (size_t)L * gdiff_layer_stride(h) * 3 * sizeof(float);
        PF_HIP(h, h->d_gdiff.reserve(need, need + need / 8, Wait::on(s)));
    }
    if ((rc = bwd_prologue(bc, dev_grad)) != PF_OK || (rc = bwd_side_lists(bc)) != PF_OK) return rc;
    bwd_head_launch(bc);
    if (bc.side_on) PF_HIP(h, h->cmp_ev[1].hold(bc.s));       // the side stream's first group
    // The last conv layer's output is read on the pharm nodes only (dynamics_gvp.py:91), the layer before it only where the last
    // one reads it (the pharm nodes and the active atoms): every other row has a zero gradient and, as in the forward, no work
    for (int l = L - 1; l >= 0; --l, bc.a ^= 1) {
        const bool last = l == L - 1;
        bwd_node_launch(bc, l);
        if (last && bc.side_on) PF_HIP(h, h->cmp_ev[2].hold(bc.s));      // the side stream's second group
        bwd_edge_levels(bc, l);
        bwd_fix_join(bc, l);
        if (bc.full && last && L >= 2 && bc.side_on && (rc = bwd_early_reduce(bc, l)) != PF_OK) return rc;
    }
    if (bc.full || bc.g_h) bwd_encoders(bc);
    if (bc.g_x) bwd_center_sum(bc);
    if (bc.full) {
        bc.rp.cls_mask = ~bc.early_mask;
        pfk_train_reduce(&bc.rp, bc.s);
        if (bc.early_mask) PF_HIP(h, h->cmp_ev[1].hold(bc.s));       // the gradient is complete on the caller's stream
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    h->tA_dirty = false;
    return PF_OK;
}

// pf_train_backward (g_pharm_x == g_pharm_h == NULL) and pf_train_backward_inputs; who: the entry, for the messages
static int train_backward(pf_handle* h, const float* dev_g_eps_h, const float* dev_g_eps_x, float* dev_grad, float* g_pharm_x,
                          float* g_pharm_h, pf_stream stream, const char* who) {
    PF_TRAIN_WIDTH_GUARD(h, who);
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!h->t_have_fwd) PF_FAIL(h, PF_ERR_STATE, "%s: no pf_train_forward on this batch", who);
    if (!dev_g_eps_h || !dev_g_eps_x || !dev_grad) PF_FAIL(h, PF_ERR_ARG, "%s: null argument", who);
    if (h->n_tseg < 0) PF_FAIL(h, PF_ERR_ARG, "%s: the gradient path supports n_convs <= 4", who);
    if ((g_pharm_x || g_pharm_h) && (rc = tuned_input_grads_guard(h, who)) != PF_OK) return rc;
    if (h->train_wide) return wide_train_backward(h, dev_g_eps_h, dev_g_eps_x, dev_grad, g_pharm_x, g_pharm_h, (hipStream_t)stream);
    return tuned_train_backward(h, dev_g_eps_h, dev_g_eps_x, dev_grad, g_pharm_x, g_pharm_h, (hipStream_t)stream);
}

int pf_train_backward(pf_handle* h, const float* dev_g_eps_h, const float* dev_g_eps_x, float* dev_grad, pf_stream stream) {
    return train_backward(h, dev_g_eps_h, dev_g_eps_x, dev_grad, nullptr, nullptr, stream, __func__);
}

int pf_train_backward_inputs(pf_handle* h, const float* dev_g_eps_h, const float* dev_g_eps_x, float* dev_grad, float* dev_g_pharm_x,
                             float* dev_g_pharm_h, pf_stream stream) {
    if (!dev_g_pharm_x && !dev_g_pharm_h) return pf_train_backward(h, dev_g_eps_h, dev_g_eps_x, dev_grad, stream);
    return train_backward(h, dev_g_eps_h, dev_g_eps_x, dev_grad, dev_g_pharm_x, dev_g_pharm_h, stream, __func__);
}

// The VJP of the dynamics w.r.t. the inputs of the kept forward alone: the selected family's backward without a parameter gradient
int pf_dynamics_input_vjp(pf_handle* h, const float* dev_g_eps_h, const float* dev_g_eps_x, float* dev_g_pharm_x, float* dev_g_pharm_h,
                          pf_stream stream) {
    PF_TRAIN_WIDTH_GUARD(h, __func__);
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!h->t_have_fwd) PF_FAIL(h, PF_ERR_STATE, "pf_dynamics_input_vjp: no pf_train_forward on this batch");
    if (!dev_g_eps_h || !dev_g_eps_x) PF_FAIL(h, PF_ERR_ARG, "pf_dynamics_input_vjp: null argument");
    if (!dev_g_pharm_x && !dev_g_pharm_h) PF_FAIL(h, PF_ERR_ARG, "pf_dynamics_input_vjp: at least one of dev_g_pharm_x / dev_g_pharm_h must be given");
    if (h->n_tseg < 0) PF_FAIL(h, PF_ERR_ARG, "pf_dynamics_input_vjp: the gradient path supports n_convs <= 4");
    if ((rc = tuned_input_grads_guard(h, __func__)) != PF_OK) return rc;
    if (!h->train_wide) return tuned_train_backward(h, dev_g_eps_h, dev_g_eps_x, nullptr, dev_g_pharm_x, dev_g_pharm_h, (hipStream_t)stream);
    return wide_train_backward(h, dev_g_eps_h, dev_g_eps_x, nullptr, dev_g_pharm_x, dev_g_pharm_h, (hipStream_t)stream);
}

// ---- guided sampling: restraint energies on the predicted clean centers steer the reverse steps (reconstruction guidance) ----
// The restraint block, its checks and its packing, and the layouts of the two workspaces a step writes: pf_restr.h (host only)
static pfrestr::GuideWork guide_work(const pf_handle* h) { return pfrestr::GuideWork(h->Nf, h->cfg.pharm_nf, h->B); }
static pfrestr::TypeWork type_work(const pf_handle* h) { return pfrestr::TypeWork(h->Nf, h->cfg.pharm_nf, h->B); }
static pfpairs::PairWork pair_work(const pf_handle* h) { return pfpairs::PairWork(h->Nf, h->B); }

int pf_sample_begin_guided(pf_handle* h, const float* dev_init_pharm_com, const float* dev_noise0, const int32_t* dev_pin_flags,
                           const float* dev_pin_x, const float* dev_pin_h, float feat_norm_constant, const int32_t* host_restr_ptr,
                           const int32_t* host_restr_kind, const int32_t* host_restr_center, const float* host_restr_p,
                           const float* host_restr_r, const float* host_restr_w, float guide_scale, float guide_clip, pf_stream stream) {
    const bool seeded = h && take(h->seed_armed), fielded = h && take(h->field.armed), typed = h && take(h->types.armed);
    const bool paired = h && take(h->pairs.armed) && h->pairs.n_arm > 0;     // (an arming without a restraint is inert: nothing of it runs)
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (fielded && typed && h->field.arm.type_sharpness != h->types.arm.type_sharpness)
        PF_FAIL(h, PF_ERR_ARG, "pf_sample_begin_guided: the pocket field's type_sharpness (%g) and the type guidance's (%g) must agree",
                (double)h->field.arm.type_sharpness, (double)h->types.arm.type_sharpness);
    if (!dev_noise0) PF_FAIL(h, PF_ERR_ARG, "pf_sample_begin_guided: null noise");
    if (!dev_pin_flags || !dev_pin_x || !dev_pin_h) PF_FAIL(h, PF_ERR_ARG, "pf_sample_begin_guided: null pin array");
    if (!(feat_norm_constant > 0.f)) PF_FAIL(h, PF_ERR_ARG, "pf_sample_begin_guided: feat_norm_constant must be positive");
    if (!h->train_wide && !(h->spec && h->train_in_grads))
        PF_FAIL(h, PF_ERR_STATE, "pf_sample_begin_guided: a guided step runs the width-generic training forward and its input gradients: "
                                 "call pf_train_set_family(h, PF_TRAIN_FAMILY_WIDE) first");
    if ((rc = tuned_input_grads_guard(h, "pf_sample_begin_guided")) != PF_OK) return rc;      // (the tuned family: fp32)
    const pfrestr::RestrArgs a{host_restr_ptr, host_restr_kind, host_restr_center, host_restr_p, host_restr_r, host_restr_w, guide_scale, guide_clip};
    char msg[256];
    if (!pfrestr::validate(a, h->B, h->h_pharm_ptr.data(), msg, sizeof msg)) PF_FAIL(h, PF_ERR_ARG, "%s", msg);
    if (const int lim = train_limits_ok(h)) return lim;
    hipStream_t s = (hipStream_t)stream;
    // every staging reservation and every device growth before anything is enqueued; the uploads behind begin_pinned
    const int n = pfrestr::n_restraints(a, h->B), nh = h->cfg.pharm_nf;
    const size_t bytes = pfrestr::RestrLayout(h->B, n).words() * 4;
    PF_HIP(h, h->restr.reserve(bytes));
    PF_HIP(h, h->restr.dev.reserve(bytes, bytes * 2, Wait::on(s)));
    const size_t gbytes = guide_work(h).words() * 4, tbytes = type_work(h).words() * 4;
    PF_HIP(h, h->d_guide.reserve(gbytes, gbytes, Wait::on(s)));
    const pffield::FieldLayout fl(h->Np, h->B, h->field.arm.n, nh);
    if (fielded) PF_HIP(h, h->field.blk.dev.reserve(fl.words() * 4, fl.words() * 8, Wait::on(s)));
    const size_t types_bytes = pftypes::TypesLayout(h->B, h->types.arm.n).words() * 4;
    if (typed) PF_HIP(h, h->types.blk.dev.reserve(types_bytes, types_bytes * 2, Wait::on(s)));
    if (typed) PF_HIP(h, h->types.d_tguide.reserve(tbytes, tbytes, Wait::on(s)));
    const size_t pairs_bytes = pfpairs::PairsLayout(h->B, h->pairs.n_arm).words() * 4, pbytes = pair_work(h).words() * 4;
    if (paired) PF_HIP(h, h->pairs.blk.dev.reserve(pairs_bytes, pairs_bytes * 2, Wait::on(s)));
    if (paired) PF_HIP(h, h->pairs.d_pguide.reserve(pbytes, pbytes, Wait::on(s)));
    rc = begin_pinned(h, dev_init_pharm_com, dev_noise0, dev_pin_flags, dev_pin_x, dev_pin_h, feat_norm_constant, seeded, stream);
    if (rc) return rc;
    pfrestr::pack(a, h->B, h->restr.stage.as<uint32_t>());
    PF_HIP(h, h->restr.upload(bytes, s));
    h->n_restr = n;
    if (fielded) {                          // the armed field becomes this run's: one copy out of the staging buffer
        PF_HIP(h, h->field.blk.upload(fl.upload_words() * 4, s));
        h->field.run = h->field.arm; h->field.on = true;
    }
    if (typed) {                            // the armed type guidance becomes this run's
        PF_HIP(h, h->types.blk.upload(types_bytes, s));
        PF_HIP(h, hipMemsetAsync(h->types.d_tguide.get(), 0, tbytes, s));
        h->types.run = h->types.arm; h->types.on = true;
    }
    if (paired) {                           // the armed pair restraints become this run's
        PF_HIP(h, h->pairs.blk.upload(pairs_bytes, s));
        h->pairs.n_run = h->pairs.n_arm; h->pairs.on = true;
    }
    PF_HIP(h, hipMemsetAsync(h->d_guide.get(), 0, gbytes, s));              // (the zero g_eps_h of every step's VJP; nothing writes it)
    h->guide_scale = guide_scale; h->guide_clip = guide_clip;
    h->guide_traj_energy = nullptr;
    h->run = RUN_GUIDED; h->guide_have = false; h->field.have = false; h->types.have = false; h->pairs.have = false;
    h->guide_wide = h->train_wide; h->guide_in_grads = h->train_in_grads;
    return PF_OK;
}

// ---- the guided step's launches: one builder per parameter struct ----
// what they share: the step's coefficients, the two workspaces and their layouts (g: d_guide; t: d_tguide, null without type guidance: no builder reads it)
struct GuideStep { float alpha_t, sigma_t; int ep_coord, ep_feat; pfrestr::GuideWork gw; float* g; pfrestr::TypeWork tw; float* t; };
static const auto guide_shared = [](const pf_handle* h, const GuideStep& st, auto& q) {      // q: GuideParams, FieldParams, TypeParams, PairParams
    q.alpha_t = st.alpha_t; q.sigma_t = st.sigma_t; q.ep_coord = st.ep_coord;
    q.D = st.g + st.gw.D(); q.g0 = st.g + st.gw.g0(); q.energy = st.g + st.gw.energy(); q.traj_energy = h->guide_traj_energy;
};
static GuideParams guide_params(const pf_handle* h, const GuideStep& st) {
    GuideParams q{};
    const pfrestr::RestrLayout rl(h->B, h->n_restr);
    const int32_t* base = h->restr.dev.as<const int32_t>();
    q.restr_ptr = base + rl.ptr(); q.restr_kind = base + rl.kind(); q.restr_center = base + rl.center();
    q.restr_p = (const float*)(base + rl.p()); q.restr_r = (const float*)(base + rl.r()); q.restr_w = (const float*)(base + rl.w());
    q.com_init = h->d_com_init;
    guide_shared(h, st, q);
    return q;
}
static FieldParams field_params(const pf_handle* h, const GuideStep& st) {
    FieldParams q{};
    const pffield::FieldLayout fl(h->Np, h->B, h->field.run.n, h->cfg.pharm_nf);
    float* fb = h->field.blk.dev.as<float>();
    q.ph_xt = (const float4*)(fb + fl.ph_xt()); q.atom_r = fb + fl.atom_r(); q.ph_ptr = (const int*)(fb + fl.ph_ptr());
    q.match = (const int*)(fb + fl.match()); q.dist = fb + fl.dist(); q.E3 = fb + fl.e3();
    const auto& r = h->field.run;
    q.w_clash = r.w_clash; q.w_comp = r.w_comp; q.kappa = r.kappa; q.type_sharpness = r.type_sharpness;
    q.ep_feat = st.ep_feat;
    guide_shared(h, st, q);
    return q;
}
static FieldTypeParams field_type_params(const pf_handle* h, const GuideStep& st) {        // unmatched, g0_h, gs_h, E_type
    return {h->types.run.unmatched, st.t + st.tw.g0_h(), st.t + st.tw.gs_h(), st.t + st.tw.E_type()};
}
// e3: the E3 of the field launch's TYPES form in front, or null
static TypeParams type_params(const pf_handle* h, const GuideStep& st, const float* e3) {
    TypeParams q{};
    const pftypes::TypesLayout tl(h->B, h->types.run.n);
    const int32_t* tb = h->types.blk.dev.as<const int32_t>();
    q.ptr = tb + tl.ptr(); q.center = tb + tl.center(); q.type = tb + tl.type();
    q.p = (const float*)(tb + tl.p()); q.r = (const float*)(tb + tl.r()); q.w = (const float*)(tb + tl.w());
    q.sharp = h->types.run.type_sharpness; q.ep_feat = st.ep_feat;
    q.g0_h = st.t + st.tw.g0_h(); q.gs_h = st.t + st.tw.gs_h(); q.E_type = st.t + st.tw.E_type(); q.E3 = e3;
    guide_shared(h, st, q);
    return q;
}
static PairParams pair_params(const pf_handle* h, const GuideStep& st) {
    PairParams q{};
    const pfpairs::PairsLayout pl(h->B, h->pairs.n_run);
    const int32_t* pb = h->pairs.blk.dev.as<const int32_t>();
    q.ptr = pb + pl.ptr(); q.i = pb + pl.i(); q.j = pb + pl.j();
    q.lo = (const float*)(pb + pl.lo()); q.hi = (const float*)(pb + pl.hi()); q.w = (const float*)(pb + pl.w());
    q.flags = h->d_pin_flags; q.pin_x = h->d_pin_x;
    const pfpairs::PairWork pw = pair_work(h);
    q.g_pair = h->pairs.d_pguide.as<float>() + pw.g_pair(); q.E_pair = h->pairs.d_pguide.as<float>() + pw.E_pair();
    guide_shared(h, st, q);
    return q;
}
static GuideShiftParams guide_shift_params(const pf_handle* h, const GuideStep& st) {      // g0, jx, D, alpha_t, sigma_t, scale, clip, grad, shift
    const pfrestr::GuideWork& w = st.gw;
    return {st.g + w.g0(), st.g + w.jx(), st.g + w.D(), st.alpha_t, st.sigma_t, h->guide_scale, h->guide_clip, st.g + w.grad(), st.g + w.shift()};
}
// live_h: a launch of this step left a g0_h (else the stored zeros stand in).  g0_h, jh, scale, clip, grad_h, shift_h
static GuideFeatParams guide_feat_params(const pf_handle* h, const GuideStep& st, bool live_h) {
    const pfrestr::TypeWork& w = st.tw;
    return {live_h ? st.t + w.g0_h() : st.g + st.gw.zero(), st.t + w.j_h(), h->types.run.feat_scale, h->types.run.feat_clip, st.t + w.grad_h(), st.t + w.shift_h()};
}

// One denoising step of a guided run: the training forward of the family the run began on (dropout 0: it keeps what the VJP reads),
// k_guide_grad, that family's inputs-only backward with g_eps_x = g0 and the zero g_eps_h, k_step_update<MoveGuided>.  The update runs
// alone: the width-generic training forward builds its own edges on every call (run_dynamics_wide: `if (!h->edges_built)`, and it
// leaves edges_built false), on a 128 / 16 handle too, and so does the tuned training forward (dyn_prologue's training forms), so no
// form of this step builds the next call's edges and edges_built stays false behind it
int pf_denoise_step_guided(pf_handle* h, const pf_step_coef* coef, const pf_pin_coef* pin, const pf_guide_coef* gc, const float* dev_noise,
                           int32_t ep_coord, int32_t ep_feat, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!coef || !pin || !gc || !dev_noise) PF_FAIL(h, PF_ERR_ARG, "pf_denoise_step_guided: null argument");
    if ((rc = run_guard(h, __func__, RUN_GUIDED)) != PF_OK) return rc;
    if (h->train_wide != h->guide_wide) PF_FAIL(h, PF_ERR_STATE, "pf_denoise_step_guided: the training family was switched inside the guided run (pf_train_set_family)");
    if (!h->train_wide && h->train_in_grads != h->guide_in_grads)
        PF_FAIL(h, PF_ERR_STATE, "pf_denoise_step_guided: the input-gradient switch was changed inside the guided run (pf_train_set_input_grads)");
    if (!h->train_wide && (rc = tuned_input_grads_guard(h, __func__)) != PF_OK) return rc;
    if (!(gc->alpha_t > 0.f)) PF_FAIL(h, PF_ERR_ARG, "pf_denoise_step_guided: alpha_t must be positive");
    hipStream_t s = (hipStream_t)stream;
    const StepParams sp = step_params(h, coef, dev_noise, ep_coord, ep_feat);
    if ((rc = train_begin(h, 0.f, 0u, s, __func__)) != PF_OK) return rc;
    h->wt_common.mask_override = nullptr;       // dropout 0, whatever a test left in pf_debug_set_dropout_masks
    h->t_common.mask_override = nullptr;
    ++h->step_id;
    h->edges_built = false; h->rec_valid = false;
    rc = run_dynamics(h, h->d_eps_h, h->d_eps_x, s, &coef->t, true, nullptr);
    h->t_have_fwd = false;                      // (the kept forward is this step's: d_t does not hold its timestep)
    if (rc) return rc;
    const GuideStep st{gc->alpha_t, gc->sigma_t, ep_coord, ep_feat, guide_work(h), h->d_guide.as<float>(), type_work(h), h->types.on ? h->types.d_tguide.as<float>() : nullptr};
    float *const g0 = st.g + st.gw.g0(), *const jx = st.g + st.gw.jx();
    const GuideParams gq = guide_params(h, st);
    pfk_guide_grad(&sp, &gq, s);
    bool comp_types = false;
    const float* e3 = nullptr;
    if (h->field.on) {                          // the pocket field adds into g0 and E (one more launch; none without a field)
        const FieldParams fq = field_params(h, st);
        comp_types = h->types.on && h->types.run.comp && h->field.run.n > 0 && h->field.run.w_comp > 0.f;
        if (comp_types) {                       // the TYPES form: the complementarity energy leaves its feature gradient too
            const FieldTypeParams ft = field_type_params(h, st);
            pfk_guide_field_types(&sp, &fq, &ft, s);
            e3 = fq.E3;
        } else pfk_guide_field(&sp, &fq, s);
    }
    h->field.have = h->field.on;
    const bool restr_types = h->types.on && h->types.run.n > 0;
    if (restr_types) {                          // type restraints: one more launch, behind the field's
        const TypeParams tq = type_params(h, st, e3);
        pfk_guide_types(&sp, &tq, s);
    }
    if (h->pairs.on) {                          // pair restraints: one more launch, the last in front of the VJP
        const PairParams pq = pair_params(h, st);
        pfk_guide_pairs(&sp, &pq, s);
    }
    h->pairs.have = h->pairs.on;
    // the VJP's g_eps_h: (phi_h / phi_x) g0_h where a launch above left one, else the stored zeros; g_pharm_h only with the arming
    const bool live_h = comp_types || restr_types;
    const float* g_eps_h = live_h ? st.t + st.tw.gs_h() : st.g + st.gw.zero();
    float* g_h = h->types.on ? st.t + st.tw.j_h() : nullptr;
    if (g_h && h->B) {
        // the encoders' backward recomputes their forward from pharm_h and d_t, and this step's forward took its timestep as a
        // scalar: d_t gets it now (nothing else reads d_t before the next call that loads it: t_have_fwd is false from here on)
        uint32_t bits; memcpy(&bits, &coef->t, 4);
        PF_HIP(h, hipMemsetD32Async((hipDeviceptr_t)h->d_t, (int)bits, (size_t)h->B, s));
    }
    rc = h->train_wide ? wide_train_backward(h, g_eps_h, g0, nullptr, jx, g_h, s) : tuned_train_backward(h, g_eps_h, g0, nullptr, jx, g_h, s);
    if (rc) return rc;
    StepMove mv;
    mv.build_form = false;
    mv.args.kind = h->types.on ? StepMoveArgs::GUIDED_TYPES : StepMoveArgs::GUIDED;
    mv.args.pin = pin_params(h, pin); mv.args.shift = guide_shift_params(h, st);
    if (h->types.on) mv.args.feat = guide_feat_params(h, st, live_h);
    h->guide_have = true;
    h->types.have = h->types.on; h->types.live = live_h;
    return step_end(h, sp, mv, s);
}

int pf_sample_guided(pf_handle* h, int32_t n_steps, const pf_step_coef* host_coef, const pf_pin_coef* host_pin_coef,
                     const pf_guide_coef* host_guide_coef, const float* dev_noise, const float* dev_init_pharm_com,
                     const int32_t* dev_pin_flags, const float* dev_pin_x, const float* dev_pin_h, int32_t ep_coord, int32_t ep_feat,
                     float feat_norm_constant, const int32_t* host_restr_ptr, const int32_t* host_restr_kind, const int32_t* host_restr_center,
                     const float* host_restr_p, const float* host_restr_r, const float* host_restr_w, float guide_scale, float guide_clip,
                     float* dev_x0, float* dev_h0, float* dev_traj_x, float* dev_traj_h, float* dev_energy, pf_stream stream) {
    SampleRun r{};
    r.kind = RUN_GUIDED; r.n_ops = n_steps; r.coef = host_coef; r.pin_coef = host_pin_coef; r.guide_coef = host_guide_coef;
    r.noise = dev_noise; r.com = dev_init_pharm_com; r.pin_flags = dev_pin_flags; r.pin_x = dev_pin_x; r.pin_h = dev_pin_h;
    r.restr_ptr = host_restr_ptr; r.restr_kind = host_restr_kind; r.restr_center = host_restr_center;
    r.restr_p = host_restr_p; r.restr_r = host_restr_r; r.restr_w = host_restr_w; r.guide_scale = guide_scale; r.guide_clip = guide_clip;
    r.ep_coord = ep_coord; r.ep_feat = ep_feat; r.feat_norm = feat_norm_constant;
    r.x0 = dev_x0; r.h0 = dev_h0; r.traj_x = dev_traj_x; r.traj_h = dev_traj_h; r.energy = dev_energy;
    return sample_loop(h, r, stream);
}

int pf_debug_last_guidance(pf_handle* h, float* dev_g0, float* dev_grad, float* dev_shift, float* dev_energy, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!h->guide_have) PF_FAIL(h, PF_ERR_STATE, "pf_debug_last_guidance: no guided step on this batch");
    hipStream_t s = (hipStream_t)stream;
    const size_t nb = (size_t)h->Nf * 3 * 4;
    const pfrestr::GuideWork gw = guide_work(h);
    const float* g = h->d_guide.as<const float>();
    if (dev_g0 && nb) PF_HIP(h, hipMemcpyAsync(dev_g0, g + gw.g0(), nb, hipMemcpyDeviceToDevice, s));
    if (dev_grad && nb) PF_HIP(h, hipMemcpyAsync(dev_grad, g + gw.grad(), nb, hipMemcpyDeviceToDevice, s));
    if (dev_shift && nb) PF_HIP(h, hipMemcpyAsync(dev_shift, g + gw.shift(), nb, hipMemcpyDeviceToDevice, s));
    if (dev_energy && h->B) PF_HIP(h, hipMemcpyAsync(dev_energy, g + gw.energy(), (size_t)h->B * 4, hipMemcpyDeviceToDevice, s));
    return PF_OK;
}

// Arms the next guided begin with a pocket field (the semantics: pfdyn.h).  Every check runs before anything is touched (pf_field.h,
// host only); then the arrays are packed into the handle's pinned staging buffer -- after the last upload out of it has been
// waited for -- and stay there until that begin uploads them on its own stream.  A run in progress reads none of it and goes on
int pf_guide_field_next(pf_handle* h, const float* host_atom_r, float w_clash, const int32_t* host_ph_ptr, const float* host_ph_x,
                        const int32_t* host_ph_type, const int32_t* host_match, const float* host_dist, float w_comp, float kappa,
                        float type_sharpness) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    const pffield::FieldArgs a{host_atom_r, w_clash, host_ph_ptr, host_ph_x, host_ph_type, host_match, host_dist, w_comp, kappa, type_sharpness};
    char msg[256];
    if (!pffield::validate(a, h->B, h->Np, h->cfg.pharm_nf, msg, sizeof msg)) PF_FAIL(h, PF_ERR_ARG, "%s", msg);
    const int n = pffield::n_features(a, h->B);
    const pffield::FieldLayout fl(h->Np, h->B, n, h->cfg.pharm_nf);
    h->field.armed = false;                 // (a field armed before and not yet used is replaced, also when the allocation below fails)
    PF_HIP(h, h->field.blk.reserve(fl.upload_words() * 4));
    pffield::pack(a, h->B, h->Np, h->cfg.pharm_nf, h->field.blk.stage.as<uint32_t>());
    h->field.arm = {n, w_clash, w_comp, kappa, type_sharpness};
    h->field.armed = true;
    return PF_OK;
}

// Arms the next guided begin with type guidance (the semantics: pfdyn.h), in pf_guide_field_next's manner: every check first
// (pf_types.h, host only), then the arrays are packed into the handle's pinned staging buffer, where they stay until that begin
// uploads them on its own stream.  A run in progress reads none of it and goes on
int pf_guide_types_next(pf_handle* h, const int32_t* host_ptr, const int32_t* host_center, const int32_t* host_type, const float* host_p,
                        const float* host_r, const float* host_w, float feat_scale, float feat_clip, float type_sharpness,
                        int32_t comp_types, float unmatched) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    const pftypes::TypesArgs a{host_ptr, host_center, host_type, host_p, host_r, host_w, feat_scale, feat_clip, type_sharpness, comp_types, unmatched};
    char msg[256];
    if (!pftypes::validate(a, h->B, h->h_pharm_ptr.data(), h->cfg.pharm_nf, msg, sizeof msg)) PF_FAIL(h, PF_ERR_ARG, "%s", msg);
    const int n = pftypes::n_restraints(a, h->B);
    h->types.armed = false;                 // (an arming not yet used is replaced, also when the allocation below fails)
    PF_HIP(h, h->types.blk.reserve(pftypes::TypesLayout(h->B, n).words() * 4));
    pftypes::pack(a, h->B, h->types.blk.stage.as<uint32_t>());
    h->types.arm = {n, feat_scale, feat_clip, type_sharpness, comp_types != 0, unmatched};
    h->types.armed = true;
    return PF_OK;
}

int pf_debug_last_type_guidance(pf_handle* h, float* dev_g0_h, float* dev_grad_h, float* dev_shift_h, float* dev_E_type, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!h->guide_have || !h->types.have) PF_FAIL(h, PF_ERR_STATE, "pf_debug_last_type_guidance: no guided step with type guidance on this batch");
    hipStream_t s = (hipStream_t)stream;
    const size_t nb = (size_t)h->Nf * (size_t)h->cfg.pharm_nf * 4;
    const pfrestr::TypeWork tw = type_work(h);
    const float* t = h->types.d_tguide.as<const float>();
    if (dev_g0_h && nb) {
        if (h->types.live) PF_HIP(h, hipMemcpyAsync(dev_g0_h, t + tw.g0_h(), nb, hipMemcpyDeviceToDevice, s));
        else PF_HIP(h, hipMemsetAsync(dev_g0_h, 0, nb, s));
    }
    if (dev_grad_h && nb) PF_HIP(h, hipMemcpyAsync(dev_grad_h, t + tw.grad_h(), nb, hipMemcpyDeviceToDevice, s));
    if (dev_shift_h && nb) PF_HIP(h, hipMemcpyAsync(dev_shift_h, t + tw.shift_h(), nb, hipMemcpyDeviceToDevice, s));
    if (dev_E_type && h->B) {
        if (h->types.live) PF_HIP(h, hipMemcpyAsync(dev_E_type, t + tw.E_type(), (size_t)h->B * 4, hipMemcpyDeviceToDevice, s));
        else PF_HIP(h, hipMemsetAsync(dev_E_type, 0, (size_t)h->B * 4, s));
    }
    return PF_OK;
}

// Arms the next guided begin with pair restraints (the semantics: pfdyn.h), in pf_guide_types_next's manner: every check first
// (pf_pairs.h, host only), then the arrays are packed into the handle's pinned staging buffer, where they stay until that begin
// uploads them on its own stream.  A run in progress reads none of it and goes on
int pf_guide_pairs_next(pf_handle* h, const int32_t* host_ptr, const int32_t* host_i, const int32_t* host_j, const float* host_lo,
                        const float* host_hi, const float* host_w) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    const pfpairs::PairsArgs a{host_ptr, host_i, host_j, host_lo, host_hi, host_w};
    char msg[256];
    if (!pfpairs::validate(a, h->B, h->h_pharm_ptr.data(), msg, sizeof msg)) PF_FAIL(h, PF_ERR_ARG, "%s", msg);
    const int n = pfpairs::n_restraints(a, h->B);
    h->pairs.armed = false;                 // (an arming not yet used is replaced, also when the allocation below fails)
    PF_HIP(h, h->pairs.blk.reserve(pfpairs::PairsLayout(h->B, n).words() * 4));
    pfpairs::pack(a, h->B, h->pairs.blk.stage.as<uint32_t>());
    h->pairs.n_arm = n;
    h->pairs.armed = true;
    return PF_OK;
}

int pf_debug_last_pairs(pf_handle* h, float* dev_g_pair, float* dev_E_pair, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!h->guide_have || !h->pairs.have) PF_FAIL(h, PF_ERR_STATE, "pf_debug_last_pairs: no guided step with pair restraints on this batch");
    hipStream_t s = (hipStream_t)stream;
    const pfpairs::PairWork pw = pair_work(h);
    const float* d = h->pairs.d_pguide.as<const float>();
    if (dev_g_pair && h->Nf) PF_HIP(h, hipMemcpyAsync(dev_g_pair, d + pw.g_pair(), (size_t)h->Nf * 3 * 4, hipMemcpyDeviceToDevice, s));
    if (dev_E_pair && h->B) PF_HIP(h, hipMemcpyAsync(dev_E_pair, d + pw.E_pair(), (size_t)h->B * 4, hipMemcpyDeviceToDevice, s));
    return PF_OK;
}

// ---- sample sets (include/pfdyn.h: "sample sets") ----
// Reads the handle's config (pharm_nf) and its own workspace, nothing else: no weights, no batch, no run state.  The call waits
// for the stream at its end: the status word (types outside [0, pharm_nf), counted by k_sset_overlap's staging) is the host's to read
static_assert(sizeof(pf_sset_opts) == sizeof(pf_sset_opts_host), "pf_sset.h restates pf_sset_opts");
int pf_sample_set_analyze(pf_handle* h, int32_t P, const int32_t* host_set_ptr, const int32_t* host_center_ptr, const float* dev_x,
                          const int32_t* dev_type, const pf_sset_opts* opts, float* dev_sim, int32_t* dev_support, int32_t* dev_label,
                          int32_t* dev_centroid, int32_t* dev_size, int32_t* dev_n_clusters, float* dev_cons_x, int32_t* dev_cons_cnt,
                          pf_stream stream) {
    if (!h) return PF_ERR_ARG;
    const pfsset::SsetArgs a{P, host_set_ptr, host_center_ptr, reinterpret_cast<const pf_sset_opts_host*>(opts)};
    char msg[256];
    if (!pfsset::validate(a, msg, sizeof msg)) PF_FAIL(h, PF_ERR_ARG, "%s", msg);
    if (!dev_x || !dev_type || !dev_support || !dev_label || !dev_centroid || !dev_size || !dev_n_clusters || !dev_cons_x || !dev_cons_cnt)
        PF_FAIL(h, PF_ERR_ARG, "pf_sample_set_analyze: null device array (only dev_sim may be NULL)");
    const pfsset::SsetPlan pl = pfsset::plan(a);
    const pfsset::SsetLayout lay(pl.P, pl.S);
    hipStream_t s = (hipStream_t)stream;
    pf_handle::SsetWork& w = h->sset;
    const size_t blk_bytes = lay.words() * 4, sim_bytes = (size_t)pl.sim_floats * 4;
    PF_HIP(h, w.blk.reserve(blk_bytes));
    PF_HIP(h, w.blk.dev.reserve(blk_bytes, blk_bytes * 2, Wait::on(s)));
    if (!dev_sim) PF_HIP(h, w.d_sim.reserve(sim_bytes, sim_bytes, Wait::on(s)));
    PF_HIP(h, w.d_status.reserve(4, 4, Wait::none()));
    PF_HIP(h, w.status_host.reserve(4, 4, Wait::none()));
    pfsset::pack(a, w.blk.stage.as<uint32_t>());
    PF_HIP(h, w.blk.upload(blk_bytes, s));
    const int32_t* d = w.blk.dev.as<const int32_t>();
    SsetParams q{};
    q.P = pl.P; q.S = pl.S; q.N = pl.N; q.nf = h->cfg.pharm_nf;
    q.set_ptr = d + lay.set_ptr(); q.sim_ptr = d + lay.sim_ptr(); q.work_ptr = d + lay.work_ptr(); q.center_ptr = d + lay.center_ptr();
    q.x = dev_x; q.type = dev_type; q.inv_2s2 = pl.inv_2s2; q.tol2 = pl.tol2; q.threshold = pl.threshold;
    q.sim = dev_sim ? dev_sim : w.d_sim.as<float>();
    q.support = dev_support; q.label = dev_label; q.centroid = dev_centroid; q.size = dev_size; q.n_clusters = dev_n_clusters;
    q.cons_x = dev_cons_x; q.cons_cnt = dev_cons_cnt; q.status = w.d_status;
    PF_HIP(h, hipMemsetAsync(w.d_status, 0, 4, s));
    PF_HIP(h, hipMemsetAsync(dev_support, 0, (size_t)pl.N * 4, s));
    PF_HIP(h, hipMemsetAsync(dev_cons_x, 0, (size_t)pl.N * 12, s));
    PF_HIP(h, hipMemsetAsync(dev_cons_cnt, 0, (size_t)pl.N * 4, s));
    pfk_sset_analyze(&q, (int)pl.work_items, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    PF_HIP(h, hipMemcpyAsync(w.status_host, w.d_status, 4, hipMemcpyDeviceToHost, s));
    PF_HIP(h, hipStreamSynchronize(s));
    if (*w.status_host != 0)
        PF_FAIL(h, PF_ERR_ARG, "pf_sample_set_analyze: %d centers have a type outside [0, %d) (counted on the device; the outputs mean nothing)",
                (int)*w.status_host, (int)h->cfg.pharm_nf);
    return PF_OK;
}

// ---- pharmacophore alignment (include/pfdyn.h: "pharmacophore alignment") ----
// The contract of pf_sample_set_analyze: the handle's config (pharm_nf) and its own workspace, nothing else; the call waits for the
// stream at its end to read the status word (types outside [0, pharm_nf), counted by k_align_self)
static_assert(sizeof(pf_align_opts) == sizeof(pf_align_opts_host), "pf_align.h restates pf_align_opts");
int pf_pharm_align(pf_handle* h, int32_t Q, const int32_t* host_q_ptr, int32_t L, const int32_t* host_l_ptr, const float* dev_qx,
                   const int32_t* dev_qtype, const float* dev_lx, const int32_t* dev_ltype, const pf_align_opts* opts, float* dev_sim,
                   int32_t* dev_matched, int32_t* dev_n_seeds, float* dev_transform, pf_stream stream) {
    if (!h) return PF_ERR_ARG;
    const pfalign::AlignArgs a{Q, host_q_ptr, L, host_l_ptr, reinterpret_cast<const pf_align_opts_host*>(opts)};
    char msg[256];
    if (!pfalign::validate(a, msg, sizeof msg)) PF_FAIL(h, PF_ERR_ARG, "%s", msg);
    if (!dev_qx || !dev_qtype || !dev_lx || !dev_ltype || !dev_sim || !dev_matched || !dev_n_seeds)
        PF_FAIL(h, PF_ERR_ARG, "pf_pharm_align: null device array (only dev_transform may be NULL)");
    const pfalign::AlignPlan pl = pfalign::plan(a);
    const pfalign::AlignLayout lay(pl.Q, pl.L);
    hipStream_t s = (hipStream_t)stream;
    pf_handle::AlignWork& w = h->align;
    const size_t blk_bytes = lay.words() * 4, self_bytes = ((size_t)pl.Q + pl.L) * 4;
    PF_HIP(h, w.blk.reserve(blk_bytes));
    PF_HIP(h, w.blk.dev.reserve(blk_bytes, blk_bytes * 2, Wait::on(s)));
    PF_HIP(h, w.d_self.reserve(self_bytes, self_bytes * 2, Wait::on(s)));
    PF_HIP(h, w.d_status.reserve(4, 4, Wait::none()));
    PF_HIP(h, w.status_host.reserve(4, 4, Wait::none()));
    pfalign::pack(a, w.blk.stage.as<uint32_t>());
    PF_HIP(h, w.blk.upload(blk_bytes, s));
    const int32_t* d = w.blk.dev.as<const int32_t>();
    AlignParams q{};
    q.Q = pl.Q; q.L = pl.L; q.nf = h->cfg.pharm_nf; q.refine = pl.refine;
    q.q_ptr = d + lay.q_ptr(); q.l_ptr = d + lay.l_ptr();
    q.qx = dev_qx; q.qt = dev_qtype; q.lx = dev_lx; q.lt = dev_ltype;
    q.inv_2s2 = pl.inv_2s2; q.tol2 = pl.tol2; q.seed_tol = pl.seed_tol; q.min_area = pl.min_area;
    q.self = w.d_self.as<float>(); q.sim = dev_sim; q.matched = dev_matched; q.n_seeds = dev_n_seeds; q.transform = dev_transform;
    q.status = w.d_status;
    PF_HIP(h, hipMemsetAsync(w.d_status, 0, 4, s));
    pfk_pharm_align(&q, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    PF_HIP(h, hipMemcpyAsync(w.status_host, w.d_status, 4, hipMemcpyDeviceToHost, s));
    PF_HIP(h, hipStreamSynchronize(s));
    if (*w.status_host != 0)
        PF_FAIL(h, PF_ERR_ARG, "pf_pharm_align: %d centers have a type outside [0, %d) (counted on the device; the outputs mean nothing)",
                (int)*w.status_host, (int)h->cfg.pharm_nf);
    return PF_OK;
}

int pf_debug_last_field(pf_handle* h, float* dev_E3, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!h->guide_have || !h->field.have) PF_FAIL(h, PF_ERR_STATE, "pf_debug_last_field: no guided step with a pocket field on this batch");
    if (!dev_E3) PF_FAIL(h, PF_ERR_ARG, "pf_debug_last_field: null argument");
    const pffield::FieldLayout fl(h->Np, h->B, h->field.run.n, h->cfg.pharm_nf);
    if (h->B) PF_HIP(h, hipMemcpyAsync(dev_E3, h->field.blk.dev.as<const float>() + fl.e3(), (size_t)h->B * 12, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PF_OK;
}

int pf_train_set_precision(pf_handle* h, int32_t precision) {
    if (!h) return PF_ERR_ARG;
    if (precision != PF_TRAIN_F32 && precision != PF_TRAIN_BF16) PF_FAIL(h, PF_ERR_ARG, "pf_train_set_precision: precision must be PF_TRAIN_F32 or PF_TRAIN_BF16");
    if (precision == PF_TRAIN_BF16 && h->train_wide) PF_FAIL(h, PF_ERR_ARG, "pf_train_set_precision: the width-generic training leg (pf_train_set_family) is fp32 only");
    h->train_bf16 = precision == PF_TRAIN_BF16;
    h->t_have_fwd = false;                       // a forward of the other precision is not this backward's
    h->t_have_loss = false;
    return PF_OK;
}

int pf_train_get_precision(pf_handle* h, int32_t* precision) {
    if (!h || !precision) return PF_ERR_ARG;
    *precision = h->train_bf16 ? PF_TRAIN_BF16 : PF_TRAIN_F32;
    return PF_OK;
}

int pf_train_set_family(pf_handle* h, int32_t family) {
    if (!h) return PF_ERR_ARG;
    if (family != PF_TRAIN_FAMILY_TUNED && family != PF_TRAIN_FAMILY_WIDE) PF_FAIL(h, PF_ERR_ARG, "pf_train_set_family: family must be PF_TRAIN_FAMILY_TUNED or PF_TRAIN_FAMILY_WIDE");
    if (family == PF_TRAIN_FAMILY_WIDE) {
        if (h->train_bf16) PF_FAIL(h, PF_ERR_ARG, "pf_train_set_family: the width-generic training leg is fp32 only (pf_train_set_precision: PF_TRAIN_BF16 is set)");
    }
    if (h->train_wide != (family == PF_TRAIN_FAMILY_WIDE)) {
        // the leg that is left gives its workspace back (several GB at a training batch); it is allocated again on that leg's next use
        (void)hipDeviceSynchronize();
        if (family == PF_TRAIN_FAMILY_WIDE) { h->d_tws.release(); h->d_tA.release(); }
        else { h->d_wtws.release(); h->d_wtA.release(); }
    }
    h->train_wide = family == PF_TRAIN_FAMILY_WIDE;
    h->t_have_fwd = false;                       // a forward of the other family is not this backward's
    h->t_have_loss = false;
    h->t_ws_ready = false; h->wt_ready = false;  // (the two legs' workspaces share the loss-buffer fields: whoever runs next carves again)
    return PF_OK;
}

int pf_train_set_input_grads(pf_handle* h, int32_t on) {
    if (!h) return PF_ERR_ARG;
    if (on != 0 && on != 1) PF_FAIL(h, PF_ERR_ARG, "pf_train_set_input_grads: on must be 0 or 1");
    if (!on && h->d_gdiff) {
        (void)hipDeviceSynchronize();            // a pass in flight may still write the rows
        h->d_gdiff.release();
    }
    h->train_in_grads = on != 0;                 // (a kept forward stays good: the forward is the same with the switch on or off)
    return PF_OK;
}

int pf_train_get_input_grads(pf_handle* h, int32_t* on) {
    if (!h || !on) return PF_ERR_ARG;
    *on = h->train_in_grads ? 1 : 0;
    return PF_OK;
}

int pf_train_get_family(pf_handle* h, int32_t* family) {
    if (!h || !family) return PF_ERR_ARG;
    *family = h->train_wide ? PF_TRAIN_FAMILY_WIDE : PF_TRAIN_FAMILY_TUNED;
    return PF_OK;
}

int pf_debug_set_dropout_masks(pf_handle* h, const float* dev_masks) {
    if (!h) return PF_ERR_ARG;
    h->t_mask_override = dev_masks;
    return PF_OK;
}

int pf_debug_dropout_mask(pf_handle* h, int32_t layer, int32_t which, float dropout_p, uint32_t seed, float* dev_out, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!dev_out || layer < 0 || layer >= h->cfg.n_convs || which < 0 || which > 1) PF_FAIL(h, PF_ERR_ARG, "pf_debug_dropout_mask: bad argument");
    TrainCommon tc{};
    tc.drop_thr = dropout_p > 0.f ? (uint32_t)std::min(4294967295.0, (double)dropout_p * 4294967296.0) : 0u;
    tc.drop_scale = 1.0f / (1.0f - dropout_p);
    tc.seed = seed;
    // element = node * columns + column: 144 columns on the specialised leg, n_hidden_scalars + vector_size on the width-generic one
    const int cols = h->train_wide ? h->cfg.n_hidden_scalars + h->cfg.vector_size : 144;
    pfk_drop_masks(&tc, (uint32_t)layer * 2u + (uint32_t)which, h->N * cols, dev_out, (hipStream_t)stream);
    return PF_OK;
}

int pf_debug_ahead(pf_handle* h, int64_t* out, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!out) PF_FAIL(h, PF_ERR_ARG, "pf_debug_ahead: null argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    PF_HIP(h, hipStreamSynchronize((hipStream_t)stream));
    const int B = h->B;
    if (h->spec_valid && h->d_pa_same && h->d_dyn_cnt) {
        std::vector<int> cnt((size_t)5 * B), same(B);
        PF_HIP(h, hipMemcpy(cnt.data(), h->d_dyn_cnt, (size_t)5 * B * 4, hipMemcpyDeviceToHost));
        PF_HIP(h, hipMemcpy(same.data(), h->d_pa_same, (size_t)B * 4, hipMemcpyDeviceToHost));
        for (int g = 0; g < B; ++g) {                      // same[g]: leading 16-slot groups of the region that still apply (BuildParams::pa_same)
            const int64_t c = cnt[(size_t)3 * B + g];
            out[1] += c;
            out[0] += std::min<int64_t>(c, (int64_t)std::min(same[g], 1 << 26) * 16);
        }
    }
    if (h->cen_valid) { out[2] = 1; out[3] = h->Nf; }
    return PF_OK;
}

int pf_debug_pa_check(pf_handle* h, int64_t* out, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!out) PF_FAIL(h, PF_ERR_ARG, "pf_debug_pa_check: null argument");
    out[0] = out[1] = out[2] = 0;
    PF_HIP(h, hipStreamSynchronize((hipStream_t)stream));
    if (h->d_pa_chk) {
        unsigned long long v[3];
        PF_HIP(h, hipMemcpy(v, h->d_pa_chk, sizeof(v), hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; ++k) out[k] = (int64_t)v[k];
    }
    return PF_OK;
}

int pf_debug_kernel_family(pf_handle* h, int32_t layer, int32_t* rows_per_wave) {
    if (!h || !rows_per_wave) return PF_ERR_ARG;
    if (layer == (int)h->last_family.size() + 3 && layer > 3) {  // four past: the item maps of the n16 launches (pf_handle::last_forms)
        *rows_per_wave = h->last_forms;
        return PF_OK;
    }
    if (layer == (int)h->last_family.size() + 2 && layer > 2) {  // three past: 1 when the last call skipped "pa" regions whose rows had been computed ahead
        *rows_per_wave = h->last_spec;
        return PF_OK;
    }
    if (layer == (int)h->last_family.size() + 1 && layer > 1) {  // two past: 1 when the last call started conv layer 0's ff / fp items from the center-hoist tables
        *rows_per_wave = h->last_cen ? 1 : 0;
        return PF_OK;
    }
    if (layer == (int)h->last_family.size() && layer > 0) {      // one past the last conv layer: 16 when the last call's head ran in the tail launch
        *rows_per_wave = h->last_tail;
        return PF_OK;
    }
    if (layer < 0 || layer >= (int)h->last_family.size()) PF_FAIL(h, PF_ERR_STATE, "pf_debug_kernel_family: no dynamics call yet, or bad layer");
    *rows_per_wave = h->last_family[layer];
    return PF_OK;
}

int pf_debug_last_eps(pf_handle* h, float* dev_eps_h, float* dev_eps_x, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (dev_eps_h) PF_HIP(h, hipMemcpyAsync(dev_eps_h, h->d_eps_h, (size_t)h->Nf * h->cfg.pharm_nf * 4, hipMemcpyDeviceToDevice, s));
    if (dev_eps_x) PF_HIP(h, hipMemcpyAsync(dev_eps_x, h->d_eps_x, (size_t)h->Nf * 3 * 4, hipMemcpyDeviceToDevice, s));
    return PF_OK;
}

int pf_debug_xchg_timeouts(pf_handle* h, int32_t* n) {
    if (!h || !n) return PF_ERR_ARG;
    *n = 0;
    if (!h->d_xstat) return PF_OK;
    PF_HIP(h, hipDeviceSynchronize());
    PF_HIP(h, hipMemcpy(n, h->d_xstat, sizeof(int32_t), hipMemcpyDeviceToHost));
    return PF_OK;
}

int pf_debug_live_memory(int64_t* n_allocations, int64_t* n_bytes) {
    if (!n_allocations || !n_bytes) return PF_ERR_ARG;
    *n_allocations = pfmem::HipRuntime::live_allocations.load();
    *n_bytes = pfmem::HipRuntime::live_bytes.load();
    return PF_OK;
}

int pf_debug_chain(pf_handle* h, int32_t kind, int32_t layer, int32_t sub, int32_t n_rows, const float* dev_s_in, const float* dev_v_in,
                   float* dev_s_out, float* dev_v_out, pf_stream stream) {
    if (h && !h->spec) PF_FAIL(h, PF_ERR_ARG, "%s: specialised to n_hidden_scalars 128 / vector_size 16", __func__);
    int rc = check_ready(h, false);
    if (rc) return rc;
    const pf_config& c = h->cfg;
    if (kind == 16 || kind == 17) {           // the message / update chain in the n16 form (pf_n16.hip); rows as for kinds 0 / 1
        n16_refresh(h, (hipStream_t)stream);
        if (n_rows < 0 || !dev_s_in || !dev_v_in || !dev_s_out || !dev_v_out) PF_FAIL(h, PF_ERR_ARG, "pf_debug_chain: bad argument");
        if (layer < 0 || layer >= c.n_convs || sub < 0 || sub > (kind == 16 ? 3 : 1)) PF_FAIL(h, PF_ERR_ARG, "pf_debug_chain: bad layer / sub index");
        if (h->pk.n16_msg.empty()) PF_FAIL(h, PF_ERR_STATE, "pf_debug_chain: this architecture has no n16 streams (needs n_message_gvps >= 2)");
        UnitParams p{};
        p.s_in = dev_s_in; p.v_in = dev_v_in; p.s_out = dev_s_out; p.v_out = dev_v_out;
        p.n = n_rows; p.kind = kind;
        if (kind == 16) { p.stream = h->d_w + h->pk.n16_msg[(size_t)layer * 4 + sub]; p.n_gvps = c.n_message_gvps; p.n16_stride = (int)h->pk.n16_msg_stride; }
        else { p.stream = h->d_w + h->pk.n16_upd[(size_t)layer * 2 + sub]; p.n_gvps = c.n_update_gvps; p.n16_stride = (int)h->pk.n16_upd_stride; }
        pfk_n16_unit(&p, (hipStream_t)stream);
        hipError_t e16 = hipGetLastError();
        if (e16 != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e16));
        return PF_OK;
    }
    if (kind < 0 || kind > 3 || n_rows < 0 || !dev_s_in || !dev_v_in || !dev_s_out || !dev_v_out) PF_FAIL(h, PF_ERR_ARG, "pf_debug_chain: bad argument");
    if (kind != 3 && (layer < 0 || layer >= c.n_convs)) PF_FAIL(h, PF_ERR_ARG, "pf_debug_chain: bad layer");
    if ((kind == 0 && (sub < 0 || sub > 3)) || ((kind == 1 || kind == 2) && (sub < 0 || sub > 3))) PF_FAIL(h, PF_ERR_ARG, "pf_debug_chain: bad sub index");
    if (h->pk.rg_msg.empty()) PF_FAIL(h, PF_ERR_STATE, "pf_debug_chain: no row-group streams (weights not committed)");
    UnitParams p{};
    p.s_in = dev_s_in; p.v_in = dev_v_in; p.s_out = dev_s_out; p.v_out = dev_v_out;
    p.n = n_rows; p.kind = kind; p.pharm_nf = c.pharm_nf;
    if (kind == 0) { p.stream = h->d_w + h->pk.rg_msg[(size_t)layer * 4 + sub]; p.n_gvps = c.n_message_gvps; }
    else if (kind == 1) {
        if (sub > 1) PF_FAIL(h, PF_ERR_ARG, "pf_debug_chain: node type 0 (prot) or 1 (pharm)");
        p.stream = h->d_w + h->pk.rg_upd[(size_t)layer * 2 + sub]; p.n_gvps = c.n_update_gvps;
    } else if (kind == 2) {           // sub: 2 * node type + (0: message_layer_norms, 1: update_layer_norms)
        const size_t* lo = &h->pk.ln_off[(size_t)(layer * 2 + (sub >> 1)) * 4];
        p.ln_w = h->d_w + lo[(sub & 1) * 2]; p.ln_b = h->d_w + lo[(sub & 1) * 2 + 1];
    } else {
        p.stream = h->d_w + h->pk.rg_upd[(size_t)(c.n_convs - 1) * 2 + 1]; p.n_gvps = c.n_noise_gvps; p.skip_gvps = c.n_update_gvps;
    }
    pfk_rg_unit(&p, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) PF_FAIL(h, PF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return PF_OK;
}

int pf_debug_l0_hoist(pf_handle* h, int32_t* rows_per_wave) {
    if (!h || !rows_per_wave) return PF_ERR_ARG;
    *rows_per_wave = h->last_hoist;
    return PF_OK;
}

int pf_profile_enable(pf_handle* h, uint32_t kernel_mask) {
    if (!h) return PF_ERR_ARG;
    h->prof_mask = kernel_mask;             // recorded events accumulate until pf_profile_read
    return PF_OK;
}

static int profile_read_range(pf_handle* h, int k0, int k1, double* total_ms, int64_t* launches, pf_stream stream) {
    if (!h || !total_ms || !launches) return PF_ERR_ARG;
    PF_HIP(h, hipStreamSynchronize((hipStream_t)stream));
    for (int k = k0; k < k1; ++k) {
        double tot = 0.0;
        for (size_t i = 0; i < h->prof_used[k]; ++i) {
            float ms = 0.f;
            hipEvent_t a, b;
            PF_HIP(h, h->prof_ev[k][i].first.get(&a));
            PF_HIP(h, h->prof_ev[k][i].second.get(&b));
            PF_HIP(h, hipEventElapsedTime(&ms, a, b));
            tot += ms;
        }
        total_ms[k - k0] = tot;
        launches[k - k0] = (int64_t)h->prof_used[k];
        h->prof_used[k] = 0;
    }
    return PF_OK;
}

int pf_profile_read(pf_handle* h, double* total_ms, int64_t* launches, pf_stream stream) {
    return profile_read_range(h, 0, pf_handle::K_BWD_HEAD, total_ms, launches, stream);
}
int pf_profile_read_train(pf_handle* h, double* total_ms, int64_t* launches, pf_stream stream) {
    return profile_read_range(h, pf_handle::K_BWD_HEAD, pf_handle::K_NUM, total_ms, launches, stream);
}

int pf_debug_counts(pf_handle* h, int64_t* out, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    if (!out) PF_FAIL(h, PF_ERR_ARG, "pf_debug_counts: null argument");
    PF_HIP(h, hipStreamSynchronize((hipStream_t)stream));
    std::vector<int> cnt((size_t)5 * h->B);
    PF_HIP(h, hipMemcpy(cnt.data(), h->d_dyn_cnt, cnt.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; ++i) out[i] = 0;
    for (int g = 0; g < h->B; ++g) {
        for (int et = 0; et < 3; ++et) out[et] += cnt[(size_t)et * h->B + g];
        out[4] += cnt[(size_t)3 * h->B + g];
        out[5] += cnt[(size_t)4 * h->B + g];
    }
    out[3] = h->Epp; out[6] = h->Nf; out[7] = h->Np;
    return PF_OK;
}

int pf_debug_work(pf_handle* h, double* flops, double* bytes, int64_t* n_edges, double* executed_flops,
                  int64_t* executed_edges, pf_stream stream) {
    int rc = check_ready(h, true);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    PF_HIP(h, hipStreamSynchronize(s));
    const pf_config& c = h->cfg;
    std::vector<int> cnt((size_t)5 * h->B);
    PF_HIP(h, hipMemcpy(cnt.data(), h->d_dyn_cnt, cnt.size() * 4, hipMemcpyDeviceToHost));
    int64_t ne[4] = {0, 0, 0, h->Epp}, n_pa = 0, n_act = 0;
    for (int g = 0; g < h->B; ++g) {
        for (int et = 0; et < 3; ++et) ne[et] += cnt[(size_t)et * h->B + g];
        n_pa += cnt[(size_t)3 * h->B + g];
        n_act += cnt[(size_t)4 * h->B + g];
    }
    const double E = (double)(ne[0] + ne[1] + ne[2] + ne[3]);
    // FLOPs at 2/MAC
    auto gvp_flops = [](int vi, int vo, int si, int so) {
        const int hd = std::max(vi, vo);
        return 2.0 * (vi * hd * 3 + hd * vo * 3 + (double)(hd + si) * so + (double)so * vo);
    };
    const double g0 = gvp_flops(17, 16, 144, 128), gg = gvp_flops(16, 16, 128, 128), gl = gvp_flops(16, 1, 128, 64);
    const double per_edge = g0 + (c.n_message_gvps - 1) * gg;
    const double per_node = c.n_update_gvps * gg;
    const double head = (c.n_noise_gvps - 1) * gg + gl + 2.0 * 64 * c.pharm_nf;
    const double enc = 2.0 * 128 * ((double)h->Np * (c.rec_nf + 1) + (double)h->Nf * (c.pharm_nf + 1));
    if (flops) *flops = c.n_convs * (E * per_edge + (double)h->N * per_node) + (double)h->Nf * head + enc;
    if (bytes) *bytes = c.n_convs * (E * 736.0 + (double)h->N * 1420.0);
    if (n_edges) for (int i = 0; i < 4; ++i) n_edges[i] = ne[i];
    // what the kernels actually compute: the last layer only feeds pharm nodes; the layer before it (when pruning
    // is on) only the active atoms
    const int pl = prune_layer(h);
    double ex = (double)h->Nf * head + enc;
    for (int l = 0; l < c.n_convs; ++l) {
        double el, nl;
        if (l == c.n_convs - 1) { el = (double)(ne[0] + ne[1]); nl = (double)h->Nf; }
        else if (l == pl) { el = (double)(ne[0] + ne[1] + ne[2] + n_pa); nl = (double)(h->Nf + n_act); }
        else { el = E; nl = (double)h->N; }
        ex += el * per_edge + nl * per_node;
        // static hoist (last call): the pp edges of layer 0 skip their first message GVP but for its gates
        // (n16 form, last_hoist == 16: the pp AND pf edges skip the h_src block of the first scalar Linear and the Vh matrix product
        // -- a type-table row and 17 x 3 multiplications instead)
        if (l == 0 && h->last_hoist == 16) ex -= (double)((l == pl ? n_pa : (l == c.n_convs - 1 ? 0 : ne[3])) + ne[1] + (h->last_cen ? ne[0] + ne[2] : 0)) * (2.0 * 128 * 128 + 2.0 * 16 * 17 * 3);
        else if (l == 0 && h->last_hoist) ex -= (double)(l == pl ? n_pa : (l == c.n_convs - 1 ? 0 : ne[3])) * (g0 - 2.0 * 128 * 16);
        if (executed_edges) executed_edges[l] = (int64_t)el;
    }
    if (executed_flops) *executed_flops = ex;
    return PF_OK;
}

}  // extern "C"
