// pf_pack.h -- the weight packer of libpfdyn: state-dict tensors in, one packed weight image out (pf_pack.cpp).
// Host only: pure index arithmetic on std::vector, no HIP runtime call and no pf_handle, so it runs (and is checked:
// tests/pack_check.cpp) without a GPU.  pf_commit_weights uploads what pack_model returns.
#pragma once
#include <hip/hip_vector_types.h>

#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pfdyn.h"

namespace pfpack {      // (the library exports its C ABI only)

struct RawTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};
typedef std::map<std::string, RawTensor> RawMap;
typedef std::vector<std::pair<std::string, std::vector<int64_t>>> TensorList;     // name, shape

extern const char* const kEtKey[4];     // pharm_ff_pharm, prot_pf_pharm, pharm_fp_prot, prot_pp_prot
extern const char* const kNtKey[2];     // prot, pharm

// ------------------------------------------------------------------------------------------------
// expected state-dict layout (mirrors the reference's module tree)
// ------------------------------------------------------------------------------------------------
struct GvpSpec { std::string prefix; int vi, vo, si, so; };
std::string conv_prefix(int layer);
GvpSpec msg_spec(const pf_config& c, int layer, int et, int j);
GvpSpec upd_spec(const pf_config& c, int layer, int nt, int j);
GvpSpec head_spec(const pf_config& c, int k);
TensorList expected_tensors(const pf_config& c);       // state-dict order: the order of the flat parameter vector

// The flat parameter vector of the gradient path (all tensors in state-dict order) and the offsets into it that the gradient
// path reads on every call, resolved once by pf_commit_weights.  param_offsets fills both from a tensor list (expected_tensors(c));
// a name the table needs that the list lacks is an error (PF_ERR_STATE, err set): no entry is ever -1.
typedef std::vector<std::pair<std::string, std::pair<size_t, size_t>>> FlatLayout;     // name -> (offset, numel)
struct ParamOffsets {
    int out_w = 0, out_b = 0;               // to_scalar_output
    int enc[2][4] = {};                     // per node type the encoder's 0.weight, 0.bias, 2.weight, 2.bias
    std::vector<int> ln;                    // [layer][nt][4]: ln1_w ln1_b ln2_w ln2_b (message_layer_norms, update_layer_norms)
    std::vector<int> gvp;                   // [for_each_gvp order][6]: Wh, Wu, to_feats_out.0.{weight, bias}, scalar_to_vector_gates.{weight, bias}
    std::vector<int> edge_fx;               // [layer][message GVP level]: k_bwd_edge_level's shape class (BwdEdgeLevelParams::fx), 0: generic
};
int param_offsets(const pf_config& c, const TensorList& tensors, FlatLayout& layout, ParamOffsets& out, std::string& err);

// every GVP in the order of the GvpW / GvpT / WideGvp tables: message GVPs [layer][etype][j], update GVPs [layer][ntype][j], the noise head's
template <typename Fn>
void for_each_gvp(const pf_config& c, Fn fn) {
    for (int l = 0; l < c.n_convs; ++l)
        for (int et = 0; et < 4; ++et)
            for (int j = 0; j < c.n_message_gvps; ++j) fn(msg_spec(c, l, et, j));
    for (int l = 0; l < c.n_convs; ++l)
        for (int nt = 0; nt < 2; ++nt)
            for (int j = 0; j < c.n_update_gvps; ++j) fn(upd_spec(c, l, nt, j));
    for (int k = 0; k < c.n_noise_gvps; ++k) fn(head_spec(c, k));
}

// offsets of one GVP's fragment blocks (the fields of GvpW) in the packed image
struct GvpOff { size_t wh, wu, wh_c, wu_c, a_main, a_main_c, b_main, a_gate, a_gate_c, b_gate; };

// Where everything sits in the packed image: offsets and strides in floats.  An offset of a block that a configuration does
// not build is 0 (a vector: empty).
struct PackLayout {
    // raw (unpacked) tensors
    size_t enc_w[2]{}, enc_b[2]{}, enc_lw[2]{}, enc_lb[2]{};
    std::vector<size_t> ln_off;             // [layer][nt][4]: ln1_w ln1_b ln2_w ln2_b
    size_t out_a = 0, out_b = 0;
    size_t enc_a = 0, enc_bf = 0;           // protein encoder as A fragments / F-layout bias (encode_pre_tile)
    size_t l0h_off = 0;                     // L0H_* block (static hoist of conv layer 0's pp messages)
    size_t l0c_off = 0;                     // L0C_* block (center hoist)
    // row-group kernels (pf_rg.hip): quad streams of the message chains [layer][etype] and update chains [layer][ntype]
    std::vector<size_t> rg_msg, rg_upd;
    std::vector<size_t> rgs_msg, rgs_upd, rgs_upd_stride;   // two-wave form: wave 0's stream; wave 1's follows *_stride floats later
    size_t rgs_msg_stride = 0;
    // n16 kernels (pf_n16.hip): per chain the four waves' quad streams, wave w's *_stride floats after wave w - 1's.
    // n16_msg: every message chain with a full first GVP (M0F: what conv layers >= 1 run, and what pf_debug_chain tests)
    std::vector<size_t> n16_msg, n16_upd;
    size_t n16_msg_stride = 0, n16_upd_stride = 0;
    // conv layer 0's message chains in their own forms: protein sources (pf, pp) start from a type-table row (M0H),
    // centers (ff, fp) have zero node vectors (M0Z)
    size_t n16_l0[4] = {0, 0, 0, 0}, n16_l0_stride[4] = {0, 0, 0, 0};
    // center hoist: M0H streams of conv layer 0's chains for EVERY etype
    size_t n16_l0h[4] = {0, 0, 0, 0}, n16_l0h_stride[4] = {0, 0, 0, 0};
    // fused launch (n_convs = 2): per etype of the last layer (ff, pf) [update chain of conv layer 0 for the source type][message chain]
    size_t n16_fused[2] = {0, 0}, n16_fused_stride[2] = {0, 0};
    // tail launch (pf_n16.hip: k_n16_tail): [update chain of the centers in the last conv layer][noise head; its last GVP padded, with to_scalar_output]
    size_t n16_tail = 0, n16_tail_stride = 0;
    // width-generic family: per GVP (for_each_gvp order) the offsets of wh, wu, wm, bm, wg, bg; to_scalar_output as stored
    std::vector<size_t> wide_off;
    size_t wide_out_w = 0, wide_out_b = 0;
    // packed elements [n16_begin, w.size()) are the n16 streams: no training kernel reads them (0: there are none)
    size_t n16_begin = 0;
};

struct PackedModel {
    std::vector<float> w;                   // the packed image; every block starts on a multiple of 64 floats
    std::vector<int> map;                   // packed element -> flat parameter index (-1: zero padding); empty above 2^24 parameters
    // -DN16_SPLIT builds: the main quads of the n16 streams hold bf16 planes, two weights per 32-bit word -- not a gather.  Per such
    // word (position in w, flat index a, flat index b, plane); map is -1 there
    std::vector<int4> split_tab;
    std::vector<GvpOff> gvp;                // for_each_gvp order; empty unless spec
    PackLayout lay;
};

// Validates raw against expected_tensors(c) and packs it.  spec: the widths of the specialised kernels (128 / 16) -- their
// fragment blocks and quad streams are built; wide: the width-generic family's packing is built; the encoders and LayerNorms
// always.  Returns PF_OK, or PF_ERR_WEIGHT / PF_ERR_STATE with err set.
int pack_model(const pf_config& c, const RawMap& raw, bool spec, bool wide, PackedModel& out, std::string& err);

// plane p (0..2) of x = p0 + p1 + p2 as a bf16 bit pattern (what a split word holds of each of its two parameters)
uint32_t n16_bf16_plane(float x, int p);

}  // namespace pfpack
