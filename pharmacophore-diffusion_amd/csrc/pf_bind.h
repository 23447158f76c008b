// pf_bind.h -- the bind planner of libpfdyn: what pf_set_pocket_batch derives from the ptr arrays, the pp edges and the
// handle's knobs (pf_bind.cpp).  Host only: pure arithmetic on std::vector and on caller-supplied memory, no HIP runtime
// call, no pf_handle and no getenv, so it runs (and is checked: tests/bind_check.cpp) without a GPU.
//   plan_batch    every argument check, the in-degrees, the regions, the tile lists and the three layouts (table
//                 section, zero section, scratch).  A failing plan has touched nothing; one rejection, "edge capacity too
//                 large", has always cost the caller its previous batch and says so (BindError::batch_lost).
//   fill_tables   writes the table section -- table_bytes of it -- into the caller's memory (the pinned staging buffer):
//                 the CSR by destination, the verified pocket-group claim and the share decision, the small tables, the
//                 host pocket rows and their one-hot verdict.
// set_pocket_batch_impl (pf_host.cpp) adopts the plan between the two: that is the point of no return.
#pragma once
#include <hip/hip_vector_types.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pfdyn.h"
#include "pf_device.h"

namespace pfbind {      // (the library exports its C ABI only)

struct BindInputs {
    pf_config cfg{};
    int B = 0;
    const int32_t *prot_ptr = nullptr, *pharm_ptr = nullptr;            // [B + 1]
    int64_t n_pp = 0;
    const int32_t *pp_src = nullptr, *pp_dst = nullptr;                 // [n_pp]
    bool host_rows = false;                                             // the pocket rows are host-resident and travel with the tables
    const float *host_prot_x = nullptr, *host_prot_h = nullptr;         // [Np][3], [Np][rec_nf] (host_rows only)
    std::vector<int> rep;                                               // the pending pocket-group claim (empty: none)
    // what the arithmetic reads of the handle
    bool spec = true, wide = false, pa_check = false;
    int edge_rec = 1;
    long n16_rows_max = 0;
    bool allow_avx2 = false;                                            // the 8-edges-per-instruction pass over sorted pp edges
};

// byte offsets, every one a multiple of 256
struct TableOff {       // relative to the table buffer
    size_t pptr, fptr, gid, reg, regact, eta, nta, esrc, edst, ins, inc, ppc, et, nt, ht, pfq, regs, pas, repb, px0, ph0;
};
struct ZeroOff {        // relative to the workspace; [0, zero_bytes) is cleared by every bind
    size_t dyn, act, flag, gnorm, need, lpart, pastamp, pasame, pacnt, pagst;
};
struct ScratchOff {     // relative to the workspace, behind the zero section
    size_t xn, fh, t, h0, h1, v0, v1, ms, mv, ms2, mv2, eh, ex, c0, c1, pre, eorig, ptype, rec, zs, ptpg, xchg, cenh, cenp, snap;
};

struct BindPlan {
    int B = 0, Np = 0, Nf = 0, N = 0;
    int64_t n_pp = 0;
    int64_t Ecap = 0;                       // end of the last region (the kernels' zero row is max(Ecap, 1))
    int max_np = 0, max_nf = 0;             // largest pocket of the batch, most centers in a graph
    bool dst_sorted = true;                 // the pp edges came grouped by destination, ascending
    std::vector<int> gid;                   // [N] graph of every node
    std::vector<int> deg;                   // [Np + 1] in-edge range starts of the destination-sorted pp edges (prefix in-degrees)
    std::vector<int> epp_g, maxdeg;         // [B] pp edges / largest pp in-degree of each graph
    std::vector<int> pfq;                   // [B] reference-booked pf edge counts (message_norm 0 with kNN pf edges), else empty
    std::vector<int> h_reg, h_cap;          // [4][B] first slot / capacity of the ff, pf, fp and pa regions
    std::vector<int> reg_act, cap_act;      // [B] the active-atom lists
    int act_total = 0;
    std::vector<EdgeTile> et_tiles, et_act;
    std::vector<NodeTile> n_tiles, h_tiles, n_act;
    int et_tile0[5] = {0, 0, 0, 0, 0}, et_tile0_act[5] = {0, 0, 0, 0, 0};
    int n_edge_tiles = 0, n_node_tiles = 0, n_head_tiles = 0, n_edge_tiles_last = 0, n_node_tiles_last = 0;
    int n_edge_tiles_act = 0, n_node_tiles_act = 0;
    bool msg2 = false;                      // a second set of message rows for the last conv layer (fused launch)
    int64_t rec_slots = 0;                  // edge records: small batches only
    TableOff t{};
    size_t index_bytes = 0, table_bytes = 0, table_total = 0;      // host-built tables / what the upload covers / with the pocket rows
    ZeroOff z{};
    size_t zero_bytes = 0;
    ScratchOff s{};
    size_t ws_bytes = 0;
};

struct FillResult {
    bool share = false;                             // tables of the sharing mode were written
    long share_rows = 0;
    std::vector<int> h_share_start, h_share_cnt;    // [B]
    int host_onehot = -1;                           // host rows: 1 every feature row is a one-hot, 0 not; -1 device rows
};

struct BindError {
    std::string msg;
    bool batch_lost = false;     // plan_batch: the rejection has always left the handle without a batch (it lies behind the point of no return)
};

// the active atoms of a graph with np atoms and nf centers: at most nf * min(pf_k, np) of them (all of them without kNN)
int active_atoms(const pf_config& c, int np, int nf);

// Returns PF_OK and fills plan, or PF_ERR_ARG with err set and plan as it was.  allow_avx2 may be set only on a CPU that has AVX2.
int plan_batch(const BindInputs& in, BindPlan& plan, BindError& err);

// Writes plan.table_bytes bytes at dst.  Returns PF_OK, or PF_ERR_ARG with err set (a false pocket-group claim).
int fill_tables(const BindPlan& plan, const BindInputs& in, void* dst, FillResult& result, BindError& err);

}  // namespace pfbind
