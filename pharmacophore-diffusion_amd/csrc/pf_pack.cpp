// pf_pack.cpp -- the weight packer (pf_pack.h): pure data movement from the state-dict tensors into the layouts the kernels read.
#include "pf_pack.h"

#include <algorithm>
#include <cstring>

#include "pf_device.h"

namespace pfpack {

const char* const kEtKey[4] = {"pharm_ff_pharm", "prot_pf_pharm", "pharm_fp_prot", "prot_pp_prot"};
const char* const kNtKey[2] = {"prot", "pharm"};

static inline int rho(int r, int hl) { return (r & 3) + 8 * (r >> 2) + 4 * hl; }

static void gvp_names(const GvpSpec& g, TensorList& out) {
    const int h = std::max(g.vi, g.vo);
    out.push_back({g.prefix + "Wh", {g.vi, h}});
    out.push_back({g.prefix + "Wu", {h, g.vo}});
    out.push_back({g.prefix + "to_feats_out.0.weight", {g.so, h + g.si}});
    out.push_back({g.prefix + "to_feats_out.0.bias", {g.so}});
    out.push_back({g.prefix + "scalar_to_vector_gates.weight", {g.vo, g.so}});
    out.push_back({g.prefix + "scalar_to_vector_gates.bias", {g.vo}});
}

std::string conv_prefix(int layer) {
    return "dynamics.noise_predictor.conv_layers." + std::to_string(layer) + ".";
}
GvpSpec msg_spec(const pf_config& c, int layer, int et, int j) {
    GvpSpec g;
    g.prefix = conv_prefix(layer) + "edge_message_fns." + kEtKey[et] + "." + std::to_string(j) + ".";
    g.vi = c.vector_size + (j == 0 ? 1 : 0);
    g.vo = c.vector_size;
    g.si = c.n_hidden_scalars + (j == 0 ? c.rbf_dim : 0);
    g.so = c.n_hidden_scalars;
    return g;
}
GvpSpec upd_spec(const pf_config& c, int layer, int nt, int j) {
    GvpSpec g;
    g.prefix = conv_prefix(layer) + "node_update_fns." + kNtKey[nt] + "." + std::to_string(j) + ".";
    g.vi = g.vo = c.vector_size;
    g.si = g.so = c.n_hidden_scalars;
    return g;
}
GvpSpec head_spec(const pf_config& c, int k) {
    GvpSpec g;
    g.prefix = "dynamics.noise_predictor.noise_predictor.gvps." + std::to_string(k) + ".";
    g.vi = c.vector_size;
    g.si = c.n_hidden_scalars;
    const bool last = k == c.n_noise_gvps - 1;
    g.vo = last ? 1 : c.vector_size;
    g.so = last ? 64 : c.n_hidden_scalars;
    return g;
}

TensorList expected_tensors(const pf_config& c) {
    TensorList v;
    const int S = c.n_hidden_scalars;
    for (int nt = 0; nt < 2; ++nt) {
        const std::string p = std::string("dynamics.") + kNtKey[nt] + "_encoder.";
        const int nf = nt ? c.pharm_nf : c.rec_nf;
        v.push_back({p + "0.weight", {S, nf + 1}});
        v.push_back({p + "0.bias", {S}});
        v.push_back({p + "2.weight", {S}});
        v.push_back({p + "2.bias", {S}});
    }
    for (int l = 0; l < c.n_convs; ++l) {
        for (int et = 0; et < 4; ++et)
            for (int j = 0; j < c.n_message_gvps; ++j) gvp_names(msg_spec(c, l, et, j), v);
        for (int nt = 0; nt < 2; ++nt) {
            for (int j = 0; j < c.n_update_gvps; ++j) gvp_names(upd_spec(c, l, nt, j), v);
            for (const char* which : {"message_layer_norms", "update_layer_norms"}) {
                const std::string p = conv_prefix(l) + which + "." + kNtKey[nt] + ".feat_norm.";
                v.push_back({p + "weight", {S}});
                v.push_back({p + "bias", {S}});
            }
        }
    }
    for (int k = 0; k < c.n_noise_gvps; ++k) gvp_names(head_spec(c, k), v);
    v.push_back({"dynamics.noise_predictor.noise_predictor.to_scalar_output.weight", {c.pharm_nf, 64}});
    v.push_back({"dynamics.noise_predictor.noise_predictor.to_scalar_output.bias", {c.pharm_nf}});
    return v;
}

int param_offsets(const pf_config& c, const TensorList& tensors, FlatLayout& layout, ParamOffsets& out, std::string& err) {
    layout.clear();
    out = ParamOffsets{};
    std::map<std::string, size_t> at;
    size_t total = 0;
    for (const auto& kv : tensors) {
        size_t numel = 1;
        for (int64_t d : kv.second) numel *= (size_t)d;
        layout.push_back({kv.first, {total, numel}});
        at[kv.first] = total;
        total += numel;
    }
    bool ok = true;
    auto off = [&](const std::string& name) {
        const auto it = at.find(name);
        if (it != at.end()) return (int)it->second;
        if (ok) err = "internal: parameter " + name + " is not in the flat layout";
        ok = false;
        return 0;
    };
    const std::string head = "dynamics.noise_predictor.noise_predictor.to_scalar_output.";
    out.out_w = off(head + "weight"); out.out_b = off(head + "bias");
    for (int nt = 0; nt < 2; ++nt) {
        const std::string p = std::string("dynamics.") + kNtKey[nt] + "_encoder.";
        int k = 0;
        for (const char* t : {"0.weight", "0.bias", "2.weight", "2.bias"}) out.enc[nt][k++] = off(p + t);
    }
    for (int l = 0; l < c.n_convs; ++l)
        for (int nt = 0; nt < 2; ++nt)
            for (const char* which : {"message_layer_norms", "update_layer_norms"}) {
                const std::string p = conv_prefix(l) + which + "." + kNtKey[nt] + ".feat_norm.";
                out.ln.push_back(off(p + "weight")); out.ln.push_back(off(p + "bias"));
            }
    for_each_gvp(c, [&](const GvpSpec& g) {
        for (const char* t : {"Wh", "Wu", "to_feats_out.0.weight", "to_feats_out.0.bias", "scalar_to_vector_gates.weight", "scalar_to_vector_gates.bias"})
            out.gvp.push_back(off(g.prefix + t));
    });
    // the two message-GVP shapes k_bwd_edge_level is instantiated for: a level whose four etypes all have one of them
    for (int l = 0; l < c.n_convs; ++l)
        for (int j = 0; j < c.n_message_gvps; ++j) {
            bool f1 = true, f2 = true;
            for (int et = 0; et < 4; ++et) {
                const GvpSpec gs = msg_spec(c, l, et, j);
                f1 = f1 && gs.vi == 16 && gs.vo == 16 && gs.si == 128 && gs.so == 128;
                f2 = f2 && gs.vi == 17 && gs.vo == 16 && gs.si == 144 && gs.so == 128;
            }
            out.edge_fx.push_back(f1 ? 1 : (f2 ? 2 : 0));
        }
    return ok ? PF_OK : PF_ERR_STATE;
}

// ------------------------------------------------------------------------------------------------
// packing into MFMA A-operand fragment order (see pf_device.h "F-layout")
// ------------------------------------------------------------------------------------------------
static size_t push(std::vector<float>& w, const std::vector<float>& v) {
    while (w.size() % 64) w.push_back(0.f);     // 256-byte alignment of every block
    const size_t off = w.size();
    w.insert(w.end(), v.begin(), v.end());
    return off;
}


// width-generic family: a Linear W [n_out][K] as the B operand of v_mfma_f32_16x16x4_f32, [tile of 16 outputs][k-step][64 lanes],
// lane l <-> W[16 t + (l & 15)][4 ks + (l >> 4)] (pf_device.h: WideGvp); zero outside the matrix
static std::vector<float> pack_wide_linear(const std::vector<float>& W, int n_out, int K) {
    const int KS = (K + 3) / 4, NT = (n_out + 15) / 16;
    std::vector<float> a((size_t)NT * KS * 64, 0.f);
    for (int t = 0; t < NT; ++t)
        for (int ks = 0; ks < KS; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int n = 16 * t + (l & 15), k = 4 * ks + (l >> 4);
                if (n < n_out && k < K) a[((size_t)t * KS + ks) * 64 + l] = W[(size_t)n * K + k];
            }
    return a;
}
// the six pieces of one GVP; appends their offsets (wh, wu, wm, bm, wg, bg) to off
static void pack_wide_gvp(const RawMap& raw, const GvpSpec& g, std::vector<float>& w, std::vector<size_t>& off) {
    const int H = std::max(g.vi, g.vo);
    off.push_back(push(w, raw.at(g.prefix + "Wh").data));
    off.push_back(push(w, raw.at(g.prefix + "Wu").data));
    off.push_back(push(w, pack_wide_linear(raw.at(g.prefix + "to_feats_out.0.weight").data, g.so, g.si + H)));
    off.push_back(push(w, raw.at(g.prefix + "to_feats_out.0.bias").data));
    off.push_back(push(w, pack_wide_linear(raw.at(g.prefix + "scalar_to_vector_gates.weight").data, g.vo, g.so)));
    off.push_back(push(w, raw.at(g.prefix + "scalar_to_vector_gates.bias").data));
}

static GvpOff pack_gvp(const pf_config& c, const RawMap& raw, const GvpSpec& g, std::vector<float>& w) {
    const int H = std::max(g.vi, g.vo);
    const int nextra = g.si - c.n_hidden_scalars;     // 16 (rbf) for the first message GVP
    const int NMO = g.so / 32;
    const int NSH = 8 + (g.vi == 17 ? 1 : 0);
    const int NKS = 64 + nextra / 2 + NSH;
    const int Kin = H + g.si;
    const RawTensor& W = raw.at(g.prefix + "to_feats_out.0.weight");   // [so][si + H]
    const RawTensor& Bv = raw.at(g.prefix + "to_feats_out.0.bias");
    const RawTensor& G = raw.at(g.prefix + "scalar_to_vector_gates.weight");   // [vo][so]
    GvpOff o;
    {   // vector channel as A fragments.  k-step t < 8: lane half hl carries input channel u(t,hl) = rho(t,hl)
        // (for a 17-channel input that is Wh row 1 + u: row 0 is the unit x_diff, fed at k-step 8 by half 0).
        const std::vector<float>& wh = raw.at(g.prefix + "Wh").data;      // [vi][H]
        const std::vector<float>& wu = raw.at(g.prefix + "Wu").data;      // [H][vo]
        const bool X = g.vi == 17;
        const int NVK = 8 + (X ? 1 : 0);
        std::vector<float> awh((size_t)NVK * 64, 0.f), awu((size_t)NVK * 64, 0.f);
        for (int t = 0; t < NVK; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, hl = lane >> 5;
                int vin, hin;                      // input channel of Wh / of Wu at this k-step for this half
                if (t < 8) { vin = (X ? 1 : 0) + rho(t, hl); hin = rho(t, hl); }
                else { vin = hl == 0 ? 0 : -1; hin = hl == 0 ? 16 : -1; }
                awh[(size_t)t * 64 + lane] = (i < H && vin >= 0) ? wh[(size_t)vin * H + i] : 0.f;
                awu[(size_t)t * 64 + lane] = (i < g.vo && hin >= 0 && hin < H) ? wu[(size_t)hin * g.vo + i] : 0.f;
            }
        o.wh = push(w, awh);
        o.wu = push(w, awu);
        // four k-steps per lane for the 4-wave kernels: [t/4][lane][t%4]
        std::vector<float> c1((size_t)3 * 64 * 4, 0.f), c2((size_t)3 * 64 * 4, 0.f);
        for (int t = 0; t < NVK; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                c1[((size_t)(t / 4) * 64 + lane) * 4 + t % 4] = awh[(size_t)t * 64 + lane];
                c2[((size_t)(t / 4) * 64 + lane) * 4 + t % 4] = awu[(size_t)t * 64 + lane];
            }
        o.wh_c = push(w, c1);
        o.wu_c = push(w, c2);
    }
    std::vector<float> a((size_t)NKS * 64 * NMO, 0.f);
    for (int ks = 0; ks < NKS; ++ks)
        for (int lane = 0; lane < 64; ++lane) {
            const int i = lane & 31, hl = lane >> 5;
            int col;
            if (ks < 64) col = 32 * (ks / 16) + rho(ks % 16, hl);
            else if (ks < 64 + nextra / 2) col = 128 + 2 * (ks - 64) + hl;
            else {                                   // sh block: k-step t carries sh[u(t,hl)]; t == 8: sh[16] on half 0
                const int t = ks - 64 - nextra / 2;
                const int idx = t < 8 ? rho(t, hl) : (hl == 0 ? 16 : -1);
                col = (idx >= 0 && idx < H) ? 128 + nextra + idx : -1;
            }
            for (int mo = 0; mo < NMO; ++mo) {
                const int row = 32 * mo + i;
                a[((size_t)ks * 64 + lane) * NMO + mo] = col >= 0 ? W.data[(size_t)row * Kin + col] : 0.f;
            }
        }
    o.a_main = push(w, a);
    {   // the same fragments per output tile, four k-steps per lane: [mo][ks/4][lane][ks%4]
        const int NKS4 = (NKS + 3) / 4;
        std::vector<float> ac((size_t)NMO * NKS4 * 64 * 4, 0.f);
        for (int ks = 0; ks < NKS; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int mo = 0; mo < NMO; ++mo)
                    ac[(((size_t)mo * NKS4 + ks / 4) * 64 + lane) * 4 + ks % 4] = a[((size_t)ks * 64 + lane) * NMO + mo];
        o.a_main_c = push(w, ac);
    }
    std::vector<float> b((size_t)2 * NMO * 16);
    for (int hl = 0; hl < 2; ++hl)
        for (int mo = 0; mo < NMO; ++mo)
            for (int r = 0; r < 16; ++r) b[(size_t)hl * NMO * 16 + mo * 16 + r] = Bv.data[32 * mo + rho(r, hl)];
    o.b_main = push(w, b);
    std::vector<float> ag((size_t)NMO * 16 * 64, 0.f);
    for (int ks = 0; ks < NMO * 16; ++ks)
        for (int lane = 0; lane < 64; ++lane) {
            const int i = lane & 31, hl = lane >> 5;
            const int k = 32 * (ks / 16) + rho(ks % 16, hl);
            ag[(size_t)ks * 64 + lane] = i < g.vo ? G.data[(size_t)i * g.so + k] : 0.f;      // rows 0..vo-1 = gates
        }
    o.a_gate = push(w, ag);
    {   // gate fragments of the wave owning output tile mo: k-steps 16*mo .. 16*mo+15 as [mo][r/4][lane][r%4]
        std::vector<float> agc((size_t)NMO * 4 * 64 * 4, 0.f);
        for (int mo = 0; mo < NMO; ++mo)
            for (int r = 0; r < 16; ++r)
                for (int lane = 0; lane < 64; ++lane)
                    agc[(((size_t)mo * 4 + r / 4) * 64 + lane) * 4 + r % 4] = ag[(size_t)(mo * 16 + r) * 64 + lane];
        o.a_gate_c = push(w, agc);
    }
    {   // gate bias in R-layout: half hl, register t <-> gate rho(t,hl)
        const std::vector<float>& bgv = raw.at(g.prefix + "scalar_to_vector_gates.bias").data;
        std::vector<float> bg(16, 0.f);
        for (int hl = 0; hl < 2; ++hl)
            for (int t = 0; t < 8; ++t) bg[(size_t)hl * 8 + t] = rho(t, hl) < g.vo ? bgv[rho(t, hl)] : 0.f;
        o.b_gate = push(w, bg);
    }
    return o;
}

// ------------------------------------------------------------------------------------------------
// Quad stream of one GVP for the row-group kernels (pf_rg.hip; schedule: rg_sched in pf_device.h).  A quad is
// [64 lanes][4 images]; an image is what one lane holds of a B operand: lane f <-> output feature f (scalar Linear),
// lane 16g + u <-> output channel u of coordinate group g (vector products, gates; g = 3 unused -> 0).
// ------------------------------------------------------------------------------------------------
// the 8 gate quads of a GVP (or to_scalar_output): K split over the lane groups, quad m, image j <-> features
// 8 (4g + j) + m of lane group g (the A block (g, j) of the SA layout)
static void pack_gate_quads_rg(const std::vector<float>& Wg, int vo, int so, std::vector<float>& out, size_t base, int q0) {
    for (int lane = 0; lane < 64; ++lane) {
        const int gq = lane >> 4, u = lane & 15;
        for (int m = 0; m < 8; ++m)
            for (int j = 0; j < 4; ++j) {
                const int feat = 8 * (4 * gq + j) + m;
                out[base + ((size_t)(q0 + m) * 64 + lane) * 4 + j] = (u < vo && feat < so) ? Wg[(size_t)u * so + feat] : 0.f;
            }
    }
}
// one block of a chain: GVP g, plus the gate quads of the GVP before it (prev) when there is one
// half >= 0: the block of wave `half` of the two-wave form (outputs 64 half .. 64 half + 63 of a 128-output scalar
// Linear; a 64-output GVP is the same block for both waves)
static void pack_gvp_rg(const pf_config& c, const RawMap& raw, const GvpSpec& g, const GvpSpec* prev, std::vector<float>& out, int half = -1) {
    const int S = c.n_hidden_scalars;
    const int H = std::max(g.vi, g.vo);
    const int nextra = g.si - S;
    const bool split = half >= 0 && g.so == 128;
    const int NH = split ? 1 : g.so / 64;             // halves of 64 outputs in this block
    const int f0 = split ? 64 * half : 0;             // first output feature of the block
    const int so_end = split ? f0 + 64 : g.so;
    const bool X17 = g.vi == 17;
    const RgSched q = rg_sched(g.vi, nextra, NH, prev != nullptr);
    const int Kin = H + g.si;
    const std::vector<float>& W = raw.at(g.prefix + "to_feats_out.0.weight").data;            // [so][si + H]
    const std::vector<float>& Bv = raw.at(g.prefix + "to_feats_out.0.bias").data;
    const std::vector<float>& bg = raw.at(g.prefix + "scalar_to_vector_gates.bias").data;
    const std::vector<float>& wh = raw.at(g.prefix + "Wh").data;                              // [vi][H]
    const std::vector<float>& wu = raw.at(g.prefix + "Wu").data;                              // [H][vo]
    const size_t base = out.size();
    out.resize(base + (size_t)q.nq * 256, 0.f);
    auto at = [&](int quad, int lane, int j) -> float& { return out[base + ((size_t)quad * 64 + lane) * 4 + j]; };
    const int v0 = X17 ? 1 : 0;                      // Wh row of node-vector channel 0 (row 0 is the unit x_diff)
    for (int lane = 0; lane < 64; ++lane) {
        const int gq = lane >> 4, u = lane & 15, qq = (lane >> 2) & 3;
        // constants: scalar bias (two halves), gate bias, Wh[0][16] on the lanes that carry xhat
        at(q.q_c, lane, 0) = f0 + lane < so_end ? Bv[f0 + lane] : 0.f;
        at(q.q_c, lane, 1) = f0 + 64 + lane < so_end ? Bv[f0 + 64 + lane] : 0.f;
        at(q.q_c, lane, 2) = u < g.vo ? bg[u] : 0.f;
        at(q.q_c, lane, 3) = (X17 && qq == 0 && gq < 3) ? wh[(size_t)0 * H + 16] : 0.f;
        if (X17) {
            at(q.q_xh, lane, 0) = gq < 3 ? wh[(size_t)0 * H + u] : 0.f;                              // xhat k-step of Vh
            at(q.q_xh, lane, 1) = (gq < 3 && u < g.vo) ? wu[(size_t)16 * g.vo + u] : 0.f;           // Vh[16] k-step of Vu
            at(q.q_xh, lane, 2) = f0 + lane < so_end ? W[(size_t)(f0 + lane) * Kin + g.si + 16] : 0.f;           // sh[16] column
            at(q.q_xh, lane, 3) = f0 + 64 + lane < so_end ? W[(size_t)(f0 + 64 + lane) * Kin + g.si + 16] : 0.f;
            for (int t = 0; t < 4; ++t) at(q.q_xh + 1, lane, t) = gq < 3 ? wh[(size_t)(1 + 4 * t + qq) * H + 16] : 0.f;
        }
        for (int t = 0; t < 4; ++t)
            for (int j = 0; j < 4; ++j) {
                at(q.q_vh + t, lane, j) = gq < 3 ? wh[(size_t)(v0 + 4 * t + j) * H + u] : 0.f;
                at(q.q_vu + t, lane, j) = (gq < 3 && u < g.vo) ? wu[(size_t)(4 * t + j) * g.vo + u] : 0.f;
            }
        for (int hh = 0; hh < NH; ++hh) {
            const int f = f0 + hh * 64 + lane;
            for (int m = 0; m < 8; ++m)
                for (int aq = 0; aq < 4; ++aq)
                    for (int j = 0; j < 4; ++j)
                        at(rg_main_quad(q, NH, (m * 4 + aq) * NH + hh), lane, j) = W[(size_t)f * Kin + 8 * (4 * aq + j) + m];
            for (int aq = 0; aq < 4; ++aq)
                for (int j = 0; j < 4; ++j) {
                    if (nextra) at(q.q_rbf + aq * NH + hh, lane, j) = W[(size_t)f * Kin + S + 4 * aq + j];
                    at(q.q_sh + aq * NH + hh, lane, j) = W[(size_t)f * Kin + g.si + 4 * aq + j];
                }
        }
    }
    if (prev) pack_gate_quads_rg(raw.at(prev->prefix + "scalar_to_vector_gates.weight").data, prev->vo, prev->so, out, base, q.q_gate);
}
// end of a chain: the gate quads of its last GVP
static void pack_flush_rg(const RawMap& raw, const GvpSpec& g, std::vector<float>& out) {
    const size_t base = out.size();
    out.resize(base + (size_t)RG_NQ_FLUSH * 256, 0.f);
    pack_gate_quads_rg(raw.at(g.prefix + "scalar_to_vector_gates.weight").data, g.vo, g.so, out, base, 0);
}
// to_scalar_output (Linear 64 -> pharm_nf) as a gate-like product: [const] [8 quads] [pad]
static void pack_out_rg(const pf_config& c, const RawMap& raw, std::vector<float>& out) {
    const RawTensor& W = raw.at("dynamics.noise_predictor.noise_predictor.to_scalar_output.weight");   // [pharm_nf][64]
    const RawTensor& Bv = raw.at("dynamics.noise_predictor.noise_predictor.to_scalar_output.bias");
    const int nf = c.pharm_nf;
    const size_t base = out.size();
    out.resize(base + (size_t)RG_NQ_OUT * 256, 0.f);
    auto at = [&](int quad, int lane, int j) -> float& { return out[base + ((size_t)quad * 64 + lane) * 4 + j]; };
    for (int lane = 0; lane < 64; ++lane) {
        const int gq = lane >> 4, u = lane & 15;
        at(0, lane, 0) = u < nf ? Bv.data[u] : 0.f;
        for (int m = 0; m < 8; ++m)
            for (int j = 0; j < 4; ++j) {
                const int feat = 8 * (4 * gq + j) + m;
                at(1 + m, lane, j) = (u < nf && feat < 64) ? W.data[(size_t)u * 64 + feat] : 0.f;
            }
    }
}

// ------------------------------------------------------------------------------------------------
// n16 kernels (pf_n16.hip; schedules: n16_sched in pf_device.h): wave w's block of GVP g.  An image is one lane's share
// of an A operand of v_mfma_f32_16x16x4_f32: lane 16 gq + i <-> output row i of the tile, k = gq of the k-step.
// Scalar k-step ks <-> input feature 16 (ks >> 2) + 4 gq + (ks & 3); vector / rbf / sh k-step r <-> channel 4 gq + r.
// ------------------------------------------------------------------------------------------------
struct N16Raw {                                  // the six tensors of a GVP with 128 scalar and 16 vector outputs (g: its dimensions)
    const std::vector<float>&W, &Bv, &Wg, &bg, &wh, &wu;
    GvpSpec g;
};
// plane p (0..2) of x = p0 + p1 + p2 as a bf16 bit pattern: round-to-nearest-even of what the earlier planes left (the device's
// n16_split8 / k_n16_split_words do the same arithmetic)
uint32_t n16_bf16_plane(float x, int p) {
    uint32_t bits = 0;
    for (int k = 0; k <= p; ++k) {
        uint32_t u; memcpy(&u, &x, 4);
        bits = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
        const uint32_t hi = bits << 16;
        float back; memcpy(&back, &hi, 4);
        x -= back;
    }
    return bits & 0xffffu;
}
static void pack_n16_raw(const N16Raw& rw, int kind, int w, std::vector<float>& out, std::vector<int4>* split_rec) {
    const GvpSpec& g = rw.g;
    const N16Sched q = n16_sched(kind);
    const int H = std::max(g.vi, g.vo), Kin = H + g.si;
    const bool m0 = kind != N16_GEN, vz = kind == N16_M0Z || kind == N16_M0H;
    const int v0 = g.vi == 17 ? 1 : 0;
    const std::vector<float>& W = rw.W;             // [so][si + H]
    const std::vector<float>& Bv = rw.Bv;
    const std::vector<float>& Wg = rw.Wg;           // [vo][so]
    const std::vector<float>& bg = rw.bg;
    const std::vector<float>& wh = rw.wh;           // [vi][H]
    const std::vector<float>& wu = rw.wu;           // [H][vo]
    const size_t base = out.size();
    out.resize(base + (size_t)q.nq * 256, 0.f);
    auto at = [&](int quad, int lane, int j) -> float& { return out[base + ((size_t)quad * 64 + lane) * 4 + j]; };
    for (int lane = 0; lane < 64; ++lane) {
        const int gq = lane >> 4, i = lane & 15;
        const int f0 = 32 * w + i, f1 = 32 * w + 16 + i;             // this lane's output rows of tile 0 / tile 1
        if (m0) {
            at(q.q_x1, lane, 0) = gq == 0 ? W[(size_t)f0 * Kin + g.si + 16] : 0.f;
            at(q.q_x1, lane, 1) = gq == 0 ? W[(size_t)f1 * Kin + g.si + 16] : 0.f;
            at(q.q_x1, lane, 2) = (gq == 0 && w < 3) ? wu[(size_t)16 * g.vo + i] : 0.f;
            at(q.q_x1, lane, 3) = gq == 0 ? wh[(size_t)0 * H + i] : (lane == 16 ? wh[(size_t)0 * H + 16] : 0.f);
        }
        for (int r = 0; r < 4; ++r) {
            if (vz) at(q.q_vh, lane, r) = wh[(size_t)0 * H + 4 * gq + r];                     // Vh = Wh[0] (x) xhat
            else if (w < 3) at(q.q_vh, lane, r) = wh[(size_t)(v0 + 4 * gq + r) * H + i];
            if (q.q_w16 >= 0 && w < 3) at(q.q_w16, lane, r) = wh[(size_t)(v0 + 4 * gq + r) * H + 16];
            at(q.q_vu, lane, r) = w < 3 ? wu[(size_t)(4 * gq + r) * g.vo + i] : bg[4 * gq + r];
        }
#if N16_SPLIT
        // main quad m = plane m % 3 of the weights of output tile (m / 3) % 2 over K chunk m / 6; a 32-bit word = elements 2 d, 2 d + 1
        if (q.q_main >= 0)
            for (int qm = 0; qm < N16_NQM; ++qm) {
                const int cch = qm / 6, tt = (qm / 3) % 2, pl = qm % 3;
                const int frow = tt ? f1 : f0;
                for (int d = 0; d < 4; ++d) {
                    float v[2];
                    for (int k = 0; k < 2; ++k) {
                        const int e = 2 * d + k;
                        v[k] = W[(size_t)frow * Kin + 16 * (2 * cch + e / 4) + 4 * gq + e % 4];
                    }
                    float& word = at(q.main_pos(qm), lane, d);
                    if (split_rec) {                 // index-valued pass: v = flat index + 1 (0: a padded row)
                        word = 0.f;
                        split_rec->push_back(make_int4((int)(&word - out.data()), (int)v[0] - 1, (int)v[1] - 1, pl));
                    } else {
                        const uint32_t bits = n16_bf16_plane(v[0], pl) | (n16_bf16_plane(v[1], pl) << 16);
                        memcpy(&word, &bits, 4);
                    }
                }
            }
#else
        if (q.q_main >= 0)
            for (int qm = 0; qm < 16; ++qm)
                for (int half = 0; half < 2; ++half) {
                    const int ks = 2 * qm + half, f = 16 * (ks >> 2) + 4 * gq + (ks & 3);
                    at(q.main_pos(qm), lane, 2 * half) = W[(size_t)f0 * Kin + f];
                    at(q.main_pos(qm), lane, 2 * half + 1) = W[(size_t)f1 * Kin + f];
                }
#endif
        for (int qq = 0; qq < 2; ++qq)
            for (int half = 0; half < 2; ++half) {
                const int r = 2 * qq + half;
                if (m0) {
                    at(q.q_rbf + qq, lane, 2 * half) = W[(size_t)f0 * Kin + PF_S + 4 * gq + r];
                    at(q.q_rbf + qq, lane, 2 * half + 1) = W[(size_t)f1 * Kin + PF_S + 4 * gq + r];
                }
                at(q.q_sh + qq, lane, 2 * half) = W[(size_t)f0 * Kin + g.si + 4 * gq + r];
                at(q.q_sh + qq, lane, 2 * half + 1) = W[(size_t)f1 * Kin + g.si + 4 * gq + r];
            }
        if (q.q_b >= 0)
            for (int r = 0; r < 4; ++r) {
                at(q.q_b, lane, r) = Bv[32 * w + 4 * gq + r];
                at(q.q_b + 1, lane, r) = Bv[32 * w + 16 + 4 * gq + r];
            }
        for (int t = 0; t < 2; ++t)
            for (int r = 0; r < 4; ++r) at(q.q_gate + t, lane, r) = Wg[(size_t)i * g.so + 32 * w + 16 * t + 4 * gq + r];
    }
}
static void pack_n16(const RawMap& raw, const GvpSpec& g, int kind, int w, std::vector<float>& out, std::vector<int4>* split_rec) {
    const N16Raw rw{raw.at(g.prefix + "to_feats_out.0.weight").data, raw.at(g.prefix + "to_feats_out.0.bias").data,
                    raw.at(g.prefix + "scalar_to_vector_gates.weight").data, raw.at(g.prefix + "scalar_to_vector_gates.bias").data,
                    raw.at(g.prefix + "Wh").data, raw.at(g.prefix + "Wu").data, g};
    pack_n16_raw(rw, kind, w, out, split_rec);
}
// The noise head's last GVP (dynamics_gvp.py:17-20: 16 vectors -> 1, 128 scalars -> 64, identity vector gate) followed by
// to_scalar_output (Linear 64 -> pharm_nf, :35,39) as ONE GEN block of the tail kernel: the GVP zero-padded to 128 scalar
// and 16 vector outputs (SiLU(0) = 0: the padded scalars feed nothing), and to_scalar_output -- a Linear on the same SiLU
// output as the gate Linear -- in the unused gate rows 1 .. pharm_nf (bias in the gate bias).  Pure data movement, like
// every packing here (the gather map of pf_set_flat_params covers it).  Needs pharm_nf <= 15.
static void pack_n16_head_last(const pf_config& c, const RawMap& raw, const GvpSpec& g, int w, std::vector<float>& out, std::vector<int4>* split_rec) {
    const int nf = c.pharm_nf, H = std::max(g.vi, g.vo), Kin = H + g.si;
    const std::vector<float>& W = raw.at(g.prefix + "to_feats_out.0.weight").data;            // [64][128 + 16]
    const std::vector<float>& Bv = raw.at(g.prefix + "to_feats_out.0.bias").data;
    const std::vector<float>& Wg = raw.at(g.prefix + "scalar_to_vector_gates.weight").data;   // [1][64]
    const std::vector<float>& bg = raw.at(g.prefix + "scalar_to_vector_gates.bias").data;
    const std::vector<float>& wu = raw.at(g.prefix + "Wu").data;                              // [16][1]
    const std::vector<float>& Wo = raw.at("dynamics.noise_predictor.noise_predictor.to_scalar_output.weight").data;   // [nf][64]
    const std::vector<float>& bo = raw.at("dynamics.noise_predictor.noise_predictor.to_scalar_output.bias").data;
    std::vector<float> W2((size_t)PF_S * Kin, 0.f), B2(PF_S, 0.f), G2((size_t)16 * PF_S, 0.f), bg2(16, 0.f), U2((size_t)H * 16, 0.f);
    for (int f = 0; f < g.so; ++f) {
        for (int k = 0; k < Kin; ++k) W2[(size_t)f * Kin + k] = W[(size_t)f * Kin + k];
        B2[f] = Bv[f];
        G2[f] = Wg[f];                                                                         // gate row 0
        for (int k = 0; k < nf; ++k) G2[(size_t)(1 + k) * PF_S + f] = Wo[(size_t)k * g.so + f];
    }
    bg2[0] = bg[0];
    for (int k = 0; k < nf; ++k) bg2[1 + k] = bo[k];
    for (int ch = 0; ch < H; ++ch) U2[(size_t)ch * 16] = wu[(size_t)ch * g.vo];
    GvpSpec g2 = g;
    g2.vo = 16; g2.so = PF_S;
    const N16Raw rw{W2, B2, G2, bg2, raw.at(g.prefix + "Wh").data, U2, g2};
    pack_n16_raw(rw, N16_GEN, w, out, split_rec);
}

// ------------------------------------------------------------------------------------------------
// The image, section by section (pack_all: their order).  Every block goes through push(): it starts on a multiple of 64 floats.
// ------------------------------------------------------------------------------------------------
// encoders, LayerNorms and to_scalar_output: as stored (the width-generic family reads these too), and for the specialised
// kernels as A fragments
static void pack_small_blocks(const pf_config& c, const RawMap& raw, bool spec, PackedModel& pm) {
    for (int nt = 0; nt < 2; ++nt) {
        const std::string p = std::string("dynamics.") + kNtKey[nt] + "_encoder.";
        {   // encoder weight transposed to [nf+1][128]: coalesced loads of one input's column
            const RawTensor& W = raw.at(p + "0.weight");
            const int K = (int)W.shape[1], S = (int)W.shape[0];
            std::vector<float> wt((size_t)K * S);
            for (int f = 0; f < S; ++f) for (int k = 0; k < K; ++k) wt[(size_t)k * S + f] = W.data[(size_t)f * K + k];
            pm.lay.enc_w[nt] = push(pm.w, wt);
        }
        pm.lay.enc_b[nt] = push(pm.w, raw.at(p + "0.bias").data);
        pm.lay.enc_lw[nt] = push(pm.w, raw.at(p + "2.weight").data);
        pm.lay.enc_lb[nt] = push(pm.w, raw.at(p + "2.bias").data);
    }
    if (spec) {   // protein encoder Linear [128][rec_nf+1] as A fragments [tile][k-step][lane]; k-step t, half hl <-> input 2t+hl
        const RawTensor& W = raw.at("dynamics.prot_encoder.0.weight");
        const RawTensor& Bv = raw.at("dynamics.prot_encoder.0.bias");
        const int K = c.rec_nf + 1, nke = (K + 1) / 2;
        std::vector<float> a((size_t)4 * nke * 64, 0.f), bf(128);
        for (int mo = 0; mo < 4; ++mo)
            for (int t = 0; t < nke; ++t)
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = lane & 31, hl = lane >> 5, k = 2 * t + hl;
                    a[((size_t)mo * nke + t) * 64 + lane] = k < K ? W.data[(size_t)(32 * mo + i) * K + k] : 0.f;
                }
        for (int hl = 0; hl < 2; ++hl)
            for (int mo = 0; mo < 4; ++mo)
                for (int r = 0; r < 16; ++r) bf[(size_t)hl * 64 + mo * 16 + r] = Bv.data[32 * mo + rho(r, hl)];
        pm.lay.enc_a = push(pm.w, a);
        pm.lay.enc_bf = push(pm.w, bf);
    }
    pm.lay.ln_off.assign((size_t)c.n_convs * 2 * 4, 0);
    for (int l = 0; l < c.n_convs; ++l)
        for (int nt = 0; nt < 2; ++nt) {
            size_t* lo = &pm.lay.ln_off[(size_t)(l * 2 + nt) * 4];
            const std::string p1 = conv_prefix(l) + "message_layer_norms." + kNtKey[nt] + ".feat_norm.";
            const std::string p2 = conv_prefix(l) + "update_layer_norms." + kNtKey[nt] + ".feat_norm.";
            lo[0] = push(pm.w, raw.at(p1 + "weight").data);
            lo[1] = push(pm.w, raw.at(p1 + "bias").data);
            lo[2] = push(pm.w, raw.at(p2 + "weight").data);
            lo[3] = push(pm.w, raw.at(p2 + "bias").data);
        }
    if (spec) {   // to_scalar_output as A fragments: K = 64 (32 k-steps), rows = outputs
        const RawTensor& W = raw.at("dynamics.noise_predictor.noise_predictor.to_scalar_output.weight");
        std::vector<float> a((size_t)32 * 64, 0.f);
        for (int ks = 0; ks < 32; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, hl = lane >> 5;
                const int k = 32 * (ks / 16) + rho(ks % 16, hl);
                a[(size_t)ks * 64 + lane] = i < c.pharm_nf ? W.data[(size_t)i * 64 + k] : 0.f;
            }
        pm.lay.out_a = push(pm.w, a);
        pm.lay.out_b = push(pm.w, raw.at("dynamics.noise_predictor.noise_predictor.to_scalar_output.bias").data);
    }
}

// static hoist of conv layer 0 (pf_device.h L0H_*): pure copies of the first pp message GVP's pieces; the center hoist's block
static void pack_hoist_blocks(const pf_config& c, const RawMap& raw, PackedModel& pm) {
    const GvpSpec g = msg_spec(c, 0, ET_PP, 0);
    const std::vector<float>& W = raw.at(g.prefix + "to_feats_out.0.weight").data;        // [128][144 + 17]
    const std::vector<float>& wh = raw.at(g.prefix + "Wh").data;                          // [17][17]
    const std::vector<float>& wu = raw.at(g.prefix + "Wu").data;                          // [17][16]
    std::vector<float> blk(L0H_SIZE, 0.f);
    if (g.vi == 17 && g.so == PF_S && g.si == PF_S + PF_R && g.vo == 16) {
        const int Kin = g.si + 17;
        for (int f = 0; f < PF_S; ++f) {
            for (int k = 0; k < PF_R; ++k) blk[L0H_WR + (size_t)k * PF_S + f] = W[(size_t)f * Kin + PF_S + k];
            for (int k = 0; k < 17; ++k) blk[L0H_WSH + (size_t)k * PF_S + f] = W[(size_t)f * Kin + g.si + k];
            for (int k = 0; k < PF_S; ++k) blk[L0H_WHT + (size_t)k * PF_S + f] = W[(size_t)f * Kin + k];
            blk[L0H_B + f] = raw.at(g.prefix + "to_feats_out.0.bias").data[f];
        }
        for (int k = 0; k < 17; ++k) blk[L0H_WH0 + k] = wh[(size_t)0 * 17 + k];
        for (int k = 0; k < 17 * 16; ++k) blk[L0H_WU + k] = wu[k];
        for (int k = 0; k < 16; ++k) blk[L0H_BG + k] = raw.at(g.prefix + "scalar_to_vector_gates.bias").data[k];
        const GvpSpec gp = msg_spec(c, 0, ET_PF, 0);                  // the pf etype's type table (n16 kernels)
        const std::vector<float>& Wp = raw.at(gp.prefix + "to_feats_out.0.weight").data;
        for (int f = 0; f < PF_S; ++f) {
            for (int k = 0; k < PF_S; ++k) blk[L0H_WHT_PF + (size_t)k * PF_S + f] = Wp[(size_t)f * Kin + k];
            blk[L0H_B_PF + f] = raw.at(gp.prefix + "to_feats_out.0.bias").data[f];
        }
    }
    pm.lay.l0h_off = push(pm.w, blk);
    // center hoist (pf_cenhoist.h): the h_src blocks and biases of the ff / fp etypes' first message GVP, k-major
    if (g.vi == 17 && g.so == PF_S && g.si == PF_S + PF_R && g.vo == 16) {
        std::vector<float> cb(L0C_SIZE, 0.f);
        const int Kin = g.si + 17;
        for (int k2 = 0; k2 < 2; ++k2) {
            const GvpSpec gc = msg_spec(c, 0, k2 == 0 ? ET_FF : ET_FP, 0);
            const std::vector<float>& Wc = raw.at(gc.prefix + "to_feats_out.0.weight").data;
            const std::vector<float>& bc = raw.at(gc.prefix + "to_feats_out.0.bias").data;
            const size_t wo = k2 == 0 ? L0C_WHT_FF : L0C_WHT_FP, bo = k2 == 0 ? L0C_B_FF : L0C_B_FP;
            for (int f = 0; f < PF_S; ++f) {
                for (int k = 0; k < PF_S; ++k) cb[wo + (size_t)k * PF_S + f] = Wc[(size_t)f * Kin + k];
                cb[bo + f] = bc[f];
            }
        }
        pm.lay.l0c_off = push(pm.w, cb);
    }
}

// row-group quad streams, one contiguous stream per chain.  The pharm update chain of the last conv layer
// comes last and is followed by the noise head's chain and to_scalar_output: the fused node + head kernel
// streams straight through.  RG_TAIL_PAD quads of padding: the prefetch ring reads ahead of the last quad used.
static void pack_rg_streams(const pf_config& c, const RawMap& raw, PackedModel& pm) {
    pm.lay.rg_msg.assign((size_t)c.n_convs * 4, 0);
    pm.lay.rg_upd.assign((size_t)c.n_convs * 2, 0);
    std::vector<float> st;
    auto flush = [&]() { const size_t off = push(pm.w, st); st.clear(); return off; };
    auto chain = [&](auto spec_of, int n, int half = -1) {   // blocks of a chain: GVP j carries the gates of GVP j - 1
        GvpSpec prev;
        for (int j = 0; j < n; ++j) {
            const GvpSpec g = spec_of(j);
            pack_gvp_rg(c, raw, g, j ? &prev : nullptr, st, half);
            prev = g;
        }
        pack_flush_rg(raw, prev, st);
    };
    for (int l = 0; l < c.n_convs; ++l)
        for (int et = 0; et < 4; ++et) {
            chain([&](int j) { return msg_spec(c, l, et, j); }, c.n_message_gvps);
            pm.lay.rg_msg[(size_t)l * 4 + et] = flush();
        }
    for (int l = 0; l < c.n_convs; ++l)
        for (int nt = 0; nt < 2; ++nt) {
            if (l == c.n_convs - 1 && nt == 1) continue;
            chain([&](int j) { return upd_spec(c, l, nt, j); }, c.n_update_gvps);
            pm.lay.rg_upd[(size_t)l * 2 + nt] = flush();
        }
    chain([&](int j) { return upd_spec(c, c.n_convs - 1, 1, j); }, c.n_update_gvps);
    chain([&](int k) { return head_spec(c, k); }, c.n_noise_gvps);
    pack_out_rg(c, raw, st);
    st.resize(st.size() + (size_t)RG_TAIL_PAD * 256, 0.f);
    pm.lay.rg_upd[(size_t)(c.n_convs - 1) * 2 + 1] = flush();
    // the same chains for the two-wave form: per chain wave 0's stream, then wave 1's
    pm.lay.rgs_msg.assign((size_t)c.n_convs * 4, 0);
    pm.lay.rgs_upd.assign((size_t)c.n_convs * 2, 0);
    pm.lay.rgs_upd_stride.assign((size_t)c.n_convs * 2, 0);
    for (int l = 0; l < c.n_convs; ++l)
        for (int et = 0; et < 4; ++et) {
            for (int half = 0; half < 2; ++half) {
                chain([&](int j) { return msg_spec(c, l, et, j); }, c.n_message_gvps, half);
                if (half == 0) pm.lay.rgs_msg_stride = st.size();
            }
            pm.lay.rgs_msg[(size_t)l * 4 + et] = flush();
        }
    for (int l = 0; l < c.n_convs; ++l)
        for (int nt = 0; nt < 2; ++nt) {
            const bool tail = l == c.n_convs - 1 && nt == 1;
            for (int half = 0; half < 2; ++half) {
                chain([&](int j) { return upd_spec(c, l, nt, j); }, c.n_update_gvps, half);
                if (tail) {
                    chain([&](int k) { return head_spec(c, k); }, c.n_noise_gvps, half);
                    pack_out_rg(c, raw, st);
                }
                if (half == 0) pm.lay.rgs_upd_stride[(size_t)l * 2 + nt] = st.size();
            }
            if (!tail) pm.lay.rgs_upd[(size_t)l * 2 + nt] = flush();
        }
    st.resize(st.size() + (size_t)RG_TAIL_PAD * 256, 0.f);
    pm.lay.rgs_upd[(size_t)(c.n_convs - 1) * 2 + 1] = flush();
}

// n16 quad streams: per chain wave 0's stream, then waves 1..3.  record: the index-valued pass of a -DN16_SPLIT build -- pack_n16_raw
// notes its bf16-plane words (positions relative to the stream being packed; pm.split_tab: relative to the image)
static void pack_n16_streams(const pf_config& c, const RawMap& raw, bool record, PackedModel& pm) {
    std::vector<int4> split_pending;
    std::vector<int4>* const split_rec = record ? &split_pending : nullptr;
    pm.lay.n16_msg.assign((size_t)c.n_convs * 4, 0);
    pm.lay.n16_upd.assign((size_t)c.n_convs * 2, 0);
    std::vector<float> st;
    auto flush16 = [&]() {       // the stream goes into the image, and what was noted about its words with it
        const size_t off = push(pm.w, st);
        for (int4 r : split_pending) { r.x += (int)off; pm.split_tab.push_back(r); }
        split_pending.clear();
        st.clear();
        return off;
    };
    // (m0_at: index of the block that is a first message GVP in the full form, M0F; -1: block 0 has kind0)
    auto chain16 = [&](auto spec_of, int n, int kind0, size_t& stride, int m0_at = -1) {
        for (int w = 0; w < 4; ++w) {
            const size_t b0 = st.size();
            for (int j = 0; j < n; ++j) pack_n16(raw, spec_of(j), j == m0_at ? N16_M0F : (j == 0 ? kind0 : N16_GEN), w, st, split_rec);
            st.resize(st.size() + (size_t)N16_TAIL_PAD * 256, 0.f);
            stride = st.size() - b0;
        }
        return flush16();
    };
    for (int l = 0; l < c.n_convs; ++l)
        for (int et = 0; et < 4; ++et)
            pm.lay.n16_msg[(size_t)l * 4 + et] = chain16([&](int j) { return msg_spec(c, l, et, j); }, c.n_message_gvps, N16_M0F, pm.lay.n16_msg_stride);
    for (int et = 0; et < 4; ++et)
        pm.lay.n16_l0[et] = chain16([&](int j) { return msg_spec(c, 0, et, j); }, c.n_message_gvps,
                                (et == ET_PP || et == ET_PF) ? N16_M0H : N16_M0Z, pm.lay.n16_l0_stride[et]);
    for (int et = 0; et < 4; ++et)      // center hoist: every etype's chain with a hoisted first block (ff / fp start from P_et rows)
        pm.lay.n16_l0h[et] = chain16([&](int j) { return msg_spec(c, 0, et, j); }, c.n_message_gvps, N16_M0H, pm.lay.n16_l0h_stride[et]);
    if (c.n_convs == 2)          // fused launch: conv layer 0's update chain of the source type, then the last layer's message chain
        for (int k = 0; k < 2; ++k) {
            const int et = k == 0 ? ET_FF : ET_PF, nt = k == 0 ? 1 : 0;
            pm.lay.n16_fused[k] = chain16([&](int j) { return j < c.n_update_gvps ? upd_spec(c, 0, nt, j) : msg_spec(c, 1, et, j - c.n_update_gvps); },
                                      c.n_update_gvps + c.n_message_gvps, N16_GEN, pm.lay.n16_fused_stride[k], c.n_update_gvps);
        }
    for (int l = 0; l < c.n_convs; ++l)
        for (int nt = 0; nt < 2; ++nt)
            pm.lay.n16_upd[(size_t)l * 2 + nt] = chain16([&](int j) { return upd_spec(c, l, nt, j); }, c.n_update_gvps, N16_GEN, pm.lay.n16_upd_stride);
    {   // tail launch: the centers' update chain of the last conv layer, then the noise head (its last GVP padded, with to_scalar_output)
        const GvpSpec hl = head_spec(c, c.n_noise_gvps - 1);
        if (c.pharm_nf <= 15 && c.n_noise_gvps >= 1 && hl.vi == 16 && hl.vo == 1 && hl.si == PF_S && hl.so == 64) {
            for (int w = 0; w < 4; ++w) {
                const size_t b0 = st.size();
                for (int j = 0; j < c.n_update_gvps; ++j) pack_n16(raw, upd_spec(c, c.n_convs - 1, 1, j), N16_GEN, w, st, split_rec);
                for (int k = 0; k + 1 < c.n_noise_gvps; ++k) pack_n16(raw, head_spec(c, k), N16_GEN, w, st, split_rec);
                pack_n16_head_last(c, raw, hl, w, st, split_rec);
                st.resize(st.size() + (size_t)N16_TAIL_PAD * 256, 0.f);
                pm.lay.n16_tail_stride = st.size() - b0;
            }
            pm.lay.n16_tail = flush16();
        }
    }
}

// one pass over raw: image, GVP offsets and layout (pm.map / pm.split_tab: pack_model)
static void pack_all(const pf_config& c, const RawMap& raw, bool spec, bool wide, bool record, PackedModel& pm) {
    if (wide) {          // width-generic family: its GVPs and to_scalar_output as stored
        for_each_gvp(c, [&](const GvpSpec& g) { pack_wide_gvp(raw, g, pm.w, pm.lay.wide_off); });
        pm.lay.wide_out_w = push(pm.w, raw.at("dynamics.noise_predictor.noise_predictor.to_scalar_output.weight").data);
        pm.lay.wide_out_b = push(pm.w, raw.at("dynamics.noise_predictor.noise_predictor.to_scalar_output.bias").data);
    }
    if (spec) for_each_gvp(c, [&](const GvpSpec& g) { pm.gvp.push_back(pack_gvp(c, raw, g, pm.w)); });
    pack_small_blocks(c, raw, spec, pm);
    if (spec) {
        pack_hoist_blocks(c, raw, pm);
        pack_rg_streams(c, raw, pm);
    }
    pm.lay.n16_begin = spec ? pm.w.size() : 0;     // everything packed from here on serves the n16 (inference-only) kernels
    if (spec && c.n_message_gvps >= 2 && c.n_update_gvps >= 1) pack_n16_streams(c, raw, record, pm);
    while (pm.w.size() % 64) pm.w.push_back(0.f);
}

int pack_model(const pf_config& c, const RawMap& raw, bool spec, bool wide, PackedModel& out, std::string& err) {
    const TensorList exp = expected_tensors(c);
    for (const auto& kv : exp) {
        auto it = raw.find(kv.first);
        if (it == raw.end()) { err = "missing weight tensor " + kv.first; return PF_ERR_WEIGHT; }
        if (it->second.shape != kv.second) { err = "wrong shape for " + kv.first; return PF_ERR_WEIGHT; }
    }
    if (raw.size() != exp.size()) {
        for (const auto& kv : raw) {
            bool found = false;
            for (const auto& e : exp) if (e.first == kv.first) { found = true; break; }
            if (!found) { err = "unexpected weight tensor " + kv.first; return PF_ERR_WEIGHT; }
        }
    }
    out = PackedModel{};
    // the packing is pure data movement (copies and zero padding), so running it on tensors whose VALUES are their own
    // flat index + 1 yields, per packed element, where it comes from: the gather map that lets pf_set_flat_params refresh
    // the packed weights on the device after an optimiser step
    RawMap index;
    size_t off = 0;
    for (const auto& kv : exp) {
        RawTensor t;
        t.shape = raw.at(kv.first).shape;
        t.data.resize(raw.at(kv.first).data.size());
        for (size_t i = 0; i < t.data.size(); ++i) t.data[i] = (float)(off + i + 1);
        off += t.data.size();
        index[kv.first] = std::move(t);
    }
    if (off < (size_t(1) << 24)) {           // indices are exact in fp32
        pack_all(c, index, spec, wide, N16_SPLIT != 0, out);
        out.map.resize(out.w.size());
        for (size_t i = 0; i < out.w.size(); ++i) out.map[i] = (int)out.w[i] - 1;      // -1: zero padding
        out.w.clear(); out.gvp.clear(); out.lay = PackLayout{};      // (the value pass packs into the same buffer; split_tab stays)
    }
    pack_all(c, raw, spec, wide, false, out);
    if (!out.map.empty() && out.map.size() != out.w.size()) { err = "internal: gather map does not match the packed weights"; return PF_ERR_STATE; }
    return PF_OK;
}

}  // namespace pfpack
