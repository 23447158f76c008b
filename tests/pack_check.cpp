// pack_check -- the weight packer (csrc/pf_pack.cpp) on the CPU: packs seeded random tensors for a handful of configurations
// and checks what a wrong index would break.  Built and run by tests/test_pack_host.py (host only, under the address and
// undefined-behaviour sanitizers; once as is and once with -DN16_SPLIT=1).  Exit status 0: every check held.
// Also the flat parameter layout and the offsets the gradient path reads per call (param_offsets), per configuration.
//   pack_check [--dump DIR]      --dump: also writes DIR/cfg<k>.w / .map / .split (the packed image, the gather map, the split table)
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pf_pack.h"
#include "pf_device.h"

using namespace pfpack;

static int g_fail = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            if (++g_fail <= 20) { printf("  FAIL: "); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                     \
    } while (0)

// value i of the seeded stream: a 32-bit integer hash (lowbias32) of the counter, 24 bits of it as a multiple of 2^-23 in [-1, 1)
static float seeded(uint32_t seed, uint32_t i) {
    uint32_t x = i + seed * 0x9E3779B9u;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return (float)(x >> 8) * (1.0f / 8388608.0f) - 1.0f;
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

struct Case { const char* name; pf_config c; bool spec, wide; };

static pf_config base_config() {
    pf_config c{};
    c.abi_version = PF_ABI_VERSION;
    c.pharm_nf = 6; c.rec_nf = 11; c.vector_size = 16; c.n_hidden_scalars = 128;
    c.n_convs = 2; c.n_message_gvps = 3; c.n_update_gvps = 2; c.n_noise_gvps = 4;
    c.rbf_dim = 16;
    return c;
}

// quads of a row-group chain (pf_pack.cpp: pack_rg_streams' chain): its GVP blocks and the flush block
template <typename SpecOf>
static size_t rg_chain_quads(const pf_config& c, SpecOf spec_of, int n, bool two_wave) {
    size_t q = 0;
    for (int j = 0; j < n; ++j) {
        const GvpSpec g = spec_of(j);
        const int nh = (two_wave && g.so == 128) ? 1 : g.so / 64;
        q += rg_sched(g.vi, g.si - c.n_hidden_scalars, nh, j > 0).nq;
    }
    return q + RG_NQ_FLUSH;
}

static void check_layout(const Case& cs, const PackedModel& pm) {
    const pf_config& c = cs.c;
    const PackLayout& L = pm.lay;
    const size_t n = pm.w.size();
    const int f0 = g_fail;
    auto blk = [&](const char* what, size_t off, size_t extent) {
        CHECK(off % 64 == 0, "%s: offset %zu is not a multiple of 64 floats", what, off);
        CHECK(off + extent <= n, "%s: [%zu, %zu) leaves the image (%zu floats)", what, off, off + extent, n);
    };
    const size_t S = (size_t)c.n_hidden_scalars;
    for (int nt = 0; nt < 2; ++nt) {
        blk("enc_w", L.enc_w[nt], ((nt ? c.pharm_nf : c.rec_nf) + 1) * S);
        blk("enc_b", L.enc_b[nt], S); blk("enc_lw", L.enc_lw[nt], S); blk("enc_lb", L.enc_lb[nt], S);
    }
    CHECK(L.ln_off.size() == (size_t)c.n_convs * 8, "ln_off has %zu entries", L.ln_off.size());
    for (size_t o : L.ln_off) blk("ln_off", o, S);
    CHECK(n % 64 == 0, "the image has %zu floats: not a multiple of 64", n);
    {   // width-generic family: six pieces per GVP (wh, wu, wm, bm, wg, bg), to_scalar_output as stored
        std::vector<GvpSpec> specs;
        for_each_gvp(c, [&](const GvpSpec& g) { specs.push_back(g); });
        CHECK(L.wide_off.size() == (cs.wide ? 6 * specs.size() : 0), "wide_off has %zu entries", L.wide_off.size());
        auto frag = [](int n_out, int K) { return (size_t)((n_out + 15) / 16) * ((K + 3) / 4) * 64; };
        for (size_t i = 0; cs.wide && 6 * i + 5 < L.wide_off.size(); ++i) {
            const GvpSpec& g = specs[i];
            const size_t* o = &L.wide_off[6 * i];
            const int H = std::max(g.vi, g.vo);
            blk("wide.wh", o[0], (size_t)g.vi * H); blk("wide.wu", o[1], (size_t)H * g.vo); blk("wide.wm", o[2], frag(g.so, g.si + H));
            blk("wide.bm", o[3], g.so); blk("wide.wg", o[4], frag(g.vo, g.so)); blk("wide.bg", o[5], g.vo);
        }
        if (cs.wide) { blk("wide_out_w", L.wide_out_w, (size_t)c.pharm_nf * 64); blk("wide_out_b", L.wide_out_b, c.pharm_nf); }
    }
    if (!cs.spec) {
        CHECK(pm.gvp.empty() && L.rg_msg.empty() && L.n16_msg.empty() && L.n16_begin == 0 && L.n16_tail == 0, "a width-generic image carries specialised blocks");
        return;
    }
    blk("enc_a", L.enc_a, (size_t)4 * ((c.rec_nf + 2) / 2) * 64); blk("enc_bf", L.enc_bf, 128);
    blk("out_a", L.out_a, 32 * 64); blk("out_b", L.out_b, c.pharm_nf);
    blk("l0h_off", L.l0h_off, L0H_SIZE);
    CHECK(L.l0c_off != 0, "no center-hoist block at the specialised widths");
    blk("l0c_off", L.l0c_off, L0C_SIZE);
    {   // fragment blocks of every GVP
        std::vector<GvpSpec> specs;
        for_each_gvp(c, [&](const GvpSpec& g) { specs.push_back(g); });
        CHECK(pm.gvp.size() == specs.size(), "%zu GvpOff entries for %zu GVPs", pm.gvp.size(), specs.size());
        for (size_t i = 0; i < specs.size() && i < pm.gvp.size(); ++i) {
            const GvpSpec& g = specs[i];
            const GvpOff& o = pm.gvp[i];
            const size_t nvk = 8 + (g.vi == 17), nmo = g.so / 32, nks = 64 + (g.si - c.n_hidden_scalars) / 2 + nvk;
            blk("gvp.wh", o.wh, nvk * 64); blk("gvp.wu", o.wu, nvk * 64); blk("gvp.wh_c", o.wh_c, 768); blk("gvp.wu_c", o.wu_c, 768);
            blk("gvp.a_main", o.a_main, nks * 64 * nmo); blk("gvp.a_main_c", o.a_main_c, nmo * ((nks + 3) / 4) * 256);
            blk("gvp.b_main", o.b_main, 2 * nmo * 16); blk("gvp.a_gate", o.a_gate, nmo * 16 * 64);
            blk("gvp.a_gate_c", o.a_gate_c, nmo * 4 * 256); blk("gvp.b_gate", o.b_gate, 16);
        }
    }
    // row-group streams; the centers' update chain of the last conv layer runs on into the noise head's chain and to_scalar_output
    const int ll = c.n_convs - 1;
    CHECK(L.rg_msg.size() == (size_t)c.n_convs * 4 && L.rgs_msg.size() == L.rg_msg.size(), "rg_msg / rgs_msg sizes");
    CHECK(L.rg_upd.size() == (size_t)c.n_convs * 2 && L.rgs_upd.size() == L.rg_upd.size() && L.rgs_upd_stride.size() == L.rg_upd.size(), "rg_upd / rgs_upd sizes");
    if (g_fail != f0) return;
    const size_t head1 = rg_chain_quads(c, [&](int k) { return head_spec(c, k); }, c.n_noise_gvps, false) + RG_NQ_OUT;
    const size_t head2 = rg_chain_quads(c, [&](int k) { return head_spec(c, k); }, c.n_noise_gvps, true) + RG_NQ_OUT;
    for (int l = 0; l < c.n_convs; ++l) {
        for (int et = 0; et < 4; ++et) {
            auto so = [&](int j) { return msg_spec(c, l, et, j); };
            blk("rg_msg", L.rg_msg[l * 4 + et], rg_chain_quads(c, so, c.n_message_gvps, false) * 256);
            const size_t st = rg_chain_quads(c, so, c.n_message_gvps, true) * 256;
            CHECK(L.rgs_msg_stride == st, "rgs_msg_stride %zu, chain %zu", L.rgs_msg_stride, st);
            blk("rgs_msg", L.rgs_msg[l * 4 + et], 2 * st);
        }
        for (int nt = 0; nt < 2; ++nt) {
            auto so = [&](int j) { return upd_spec(c, l, nt, j); };
            const bool tail = l == ll && nt == 1;
            const size_t q1 = rg_chain_quads(c, so, c.n_update_gvps, false) + (tail ? head1 + RG_TAIL_PAD : 0);
            const size_t q2 = rg_chain_quads(c, so, c.n_update_gvps, true) + (tail ? head2 : 0);
            blk("rg_upd", L.rg_upd[l * 2 + nt], q1 * 256);
            CHECK(L.rgs_upd_stride[l * 2 + nt] == q2 * 256, "rgs_upd_stride[%d][%d] %zu, chain %zu", l, nt, L.rgs_upd_stride[l * 2 + nt], q2 * 256);
            blk("rgs_upd", L.rgs_upd[l * 2 + nt], (2 * q2 + (tail ? RG_TAIL_PAD : 0)) * 256);
        }
    }
    // n16 streams: four waves' streams per chain, a stride apart; every stream ends in N16_TAIL_PAD quads of read-ahead padding
    const size_t gen = n16_sched(N16_GEN).nq, m0f = n16_sched(N16_M0F).nq, m0z = n16_sched(N16_M0Z).nq, m0h = n16_sched(N16_M0H).nq;
    const size_t nm = c.n_message_gvps, nu = c.n_update_gvps;
    size_t first = n;
    auto stream = [&](const char* what, size_t off, size_t stride, size_t quads) {
        CHECK(stride == (quads + N16_TAIL_PAD) * 256, "%s: stride %zu, blocks + padding %zu", what, stride, (quads + N16_TAIL_PAD) * 256);
        blk(what, off, 4 * stride);
        first = std::min(first, off);
    };
    CHECK(L.n16_msg.size() == (size_t)c.n_convs * 4 && L.n16_upd.size() == (size_t)c.n_convs * 2, "n16_msg / n16_upd sizes");
    if (g_fail != f0) return;
    for (size_t k = 0; k < L.n16_msg.size(); ++k) stream("n16_msg", L.n16_msg[k], L.n16_msg_stride, m0f + (nm - 1) * gen);
    for (size_t k = 0; k < L.n16_upd.size(); ++k) stream("n16_upd", L.n16_upd[k], L.n16_upd_stride, nu * gen);
    for (int et = 0; et < 4; ++et) {
        stream("n16_l0", L.n16_l0[et], L.n16_l0_stride[et], ((et == ET_PP || et == ET_PF) ? m0h : m0z) + (nm - 1) * gen);
        stream("n16_l0h", L.n16_l0h[et], L.n16_l0h_stride[et], m0h + (nm - 1) * gen);
    }
    for (int k = 0; k < 2; ++k) {
        if (c.n_convs == 2) stream("n16_fused", L.n16_fused[k], L.n16_fused_stride[k], nu * gen + m0f + (nm - 1) * gen);
        else CHECK(L.n16_fused[k] == 0, "a fused stream without two conv layers");
    }
    if (c.pharm_nf <= 15) stream("n16_tail", L.n16_tail, L.n16_tail_stride, (nu + c.n_noise_gvps) * gen);
    else CHECK(L.n16_tail == 0 && L.n16_tail_stride == 0, "a tail stream at pharm_nf = %d", c.pharm_nf);
    CHECK(L.n16_begin == first, "n16_begin %zu, first n16 stream at %zu", L.n16_begin, first);
}

static void check_values(const Case& cs, const PackedModel& pm, const std::vector<float>& flat, const TensorList& exp) {
    const size_t n = pm.w.size(), np = flat.size();
    CHECK(pm.map.size() == n, "the gather map has %zu entries for %zu packed elements", pm.map.size(), n);
    if (pm.map.size() != n) return;
    std::vector<char> is_split(n, 0), seen(np, 0);
    const int f0 = g_fail;
#if N16_SPLIT
    CHECK(!cs.spec || !pm.split_tab.empty(), "a split build without a split table");
#else
    CHECK(pm.split_tab.empty(), "a split table (%zu words) in the default build", pm.split_tab.size());
#endif
    for (const int4& r : pm.split_tab) {            // (word position, flat index a, flat index b, plane); -1: a zero
        CHECK(r.x >= 0 && (size_t)r.x < n && r.y >= -1 && r.y < (int)np && r.z >= -1 && r.z < (int)np && r.w >= 0 && r.w < 3,
              "split entry (%d, %d, %d, %d) out of range", r.x, r.y, r.z, r.w);
        if (g_fail != f0) return;
        is_split[r.x] = 1;
        const uint32_t want = n16_bf16_plane(r.y >= 0 ? flat[r.y] : 0.f, r.w) | (n16_bf16_plane(r.z >= 0 ? flat[r.z] : 0.f, r.w) << 16);
        CHECK(bits(pm.w[r.x]) == want, "split word %d: %08x, planes %d of parameters %d, %d give %08x", r.x, bits(pm.w[r.x]), r.w, r.y, r.z, want);
        CHECK(pm.map[r.x] == -1, "split word %d is also gathered (map %d)", r.x, pm.map[r.x]);
        if (r.y >= 0) seen[r.y] = 1;
        if (r.z >= 0) seen[r.z] = 1;
    }
    for (size_t i = 0; i < n; ++i) {
        if (is_split[i]) continue;
        const int m = pm.map[i];
        CHECK(m >= -1 && m < (int)np, "map[%zu] = %d out of range", i, m);
        if (m < -1 || m >= (int)np) return;
        if (m < 0) CHECK(bits(pm.w[i]) == 0, "w[%zu] = %08x is padding (map -1) but not +0.0f", i, bits(pm.w[i]));
        else { CHECK(bits(pm.w[i]) == bits(flat[m]), "w[%zu] = %08x, flat[%d] = %08x", i, bits(pm.w[i]), m, bits(flat[m])); seen[m] = 1; }
    }
    if (cs.spec) {          // at the specialised widths every parameter reaches the image
        size_t off = 0;
        for (const auto& kv : exp) {
            size_t numel = 1;
            for (int64_t d : kv.second) numel *= (size_t)d;
            for (size_t i = 0; i < numel; ++i)
                if (!seen[off + i]) { CHECK(false, "parameter %zu (%s[%zu]) occurs nowhere in the packed image", off + i, kv.first.c_str(), i); break; }
            off += numel;
        }
    }
}

// The flat layout and the table of offsets the gradient path reads (param_offsets): every entry against a lookup by name that
// walks the layout, the layout against the cumulative sizes of the expected tensors, every shape class against msg_spec
static void check_offsets(const Case& cs, const TensorList& exp) {
    const pf_config& c = cs.c;
    FlatLayout lay;
    ParamOffsets po;
    std::string err;
    const int rc = param_offsets(c, exp, lay, po, err);
    CHECK(rc == PF_OK && err.empty(), "param_offsets: %d (%s)", rc, err.c_str());
    if (rc != PF_OK) return;
    CHECK(lay.size() == exp.size(), "the layout has %zu tensors, expected %zu", lay.size(), exp.size());
    size_t off = 0;
    for (size_t i = 0; i < exp.size() && i < lay.size(); ++i) {
        size_t numel = 1;
        for (int64_t d : exp[i].second) numel *= (size_t)d;
        CHECK(lay[i].first == exp[i].first && lay[i].second.first == off && lay[i].second.second == numel, "layout[%zu] = (%s, %zu, %zu), expected (%s, %zu, %zu)",
              i, lay[i].first.c_str(), lay[i].second.first, lay[i].second.second, exp[i].first.c_str(), off, numel);
        off += numel;
    }
    auto at = [&](const std::string& name) {
        for (const auto& kv : lay) if (kv.first == name) return (long)kv.second.first;
        CHECK(false, "%s is not in the layout", name.c_str());
        return -1L;
    };
    auto same = [&](const char* what, int got, const std::string& name) { CHECK(got >= 0 && (long)got == at(name), "%s = %d, %s sits at %ld", what, got, name.c_str(), at(name)); };
    const std::string head = "dynamics.noise_predictor.noise_predictor.to_scalar_output.";
    same("out_w", po.out_w, head + "weight"); same("out_b", po.out_b, head + "bias");
    const char* const enc_t[4] = {"0.weight", "0.bias", "2.weight", "2.bias"};
    for (int nt = 0; nt < 2; ++nt)
        for (int k = 0; k < 4; ++k) same("enc", po.enc[nt][k], std::string("dynamics.") + kNtKey[nt] + "_encoder." + enc_t[k]);
    CHECK(po.ln.size() == (size_t)c.n_convs * 8, "ln has %zu entries", po.ln.size());
    const char* const ln_t[4] = {"message_layer_norms", "message_layer_norms", "update_layer_norms", "update_layer_norms"};
    for (size_t i = 0; i < po.ln.size(); ++i) {
        const int l = (int)(i / 8), nt = (int)(i / 4 % 2), k = (int)(i % 4);
        same("ln", po.ln[i], conv_prefix(l) + ln_t[k] + "." + kNtKey[nt] + ".feat_norm." + (k % 2 ? "bias" : "weight"));
    }
    std::vector<GvpSpec> specs;
    for_each_gvp(c, [&](const GvpSpec& g) { specs.push_back(g); });
    CHECK(po.gvp.size() == 6 * specs.size(), "gvp has %zu entries for %zu GVPs", po.gvp.size(), specs.size());
    const char* const gvp_t[6] = {"Wh", "Wu", "to_feats_out.0.weight", "to_feats_out.0.bias", "scalar_to_vector_gates.weight", "scalar_to_vector_gates.bias"};
    for (size_t i = 0; i < po.gvp.size() && i < 6 * specs.size(); ++i) same("gvp", po.gvp[i], specs[i / 6].prefix + gvp_t[i % 6]);
    // shape classes: 1 = every etype's GVP is (16, 16, 128, 128), 2 = (17, 16, 144, 128), else 0 -- at other widths always 0
    CHECK(po.edge_fx.size() == (size_t)c.n_convs * c.n_message_gvps, "edge_fx has %zu entries", po.edge_fx.size());
    for (size_t i = 0; i < po.edge_fx.size(); ++i) {
        const int l = (int)i / c.n_message_gvps, j = (int)i % c.n_message_gvps;
        int cls = -1;
        for (int et = 0; et < 4; ++et) {
            const GvpSpec g = msg_spec(c, l, et, j);
            const int k = (g.vi == 16 && g.vo == 16 && g.si == 128 && g.so == 128) ? 1 : ((g.vi == 17 && g.vo == 16 && g.si == 144 && g.so == 128) ? 2 : 0);
            cls = (et == 0 || cls == k) ? k : 0;
        }
        CHECK(po.edge_fx[i] == cls, "edge_fx[%d][%d] = %d, msg_spec says %d", l, j, po.edge_fx[i], cls);
        if (!cs.spec) CHECK(po.edge_fx[i] == 0, "edge_fx[%d][%d] = %d at widths %d / %d", l, j, po.edge_fx[i], c.n_hidden_scalars, c.vector_size);
        else CHECK(po.edge_fx[i] == (j == 0 ? 2 : 1), "edge_fx[%d][%d] = %d at the specialised widths", l, j, po.edge_fx[i]);
    }
}

static void dump(const std::string& path, const void* p, size_t bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) { printf("cannot write %s\n", path.c_str()); ++g_fail; }
    if (f) fclose(f);
}

int main(int argc, char** argv) {
    const char* dump_dir = (argc == 3 && !strcmp(argv[1], "--dump")) ? argv[2] : nullptr;
    std::vector<Case> cases;
    {
        pf_config c = base_config();
        cases.push_back({"defaults 128/16, two conv layers", c, true, false});
        c = base_config(); c.n_convs = 1;
        cases.push_back({"one conv layer", c, true, false});
        c = base_config(); c.n_convs = 3; c.n_noise_gvps = 3;
        cases.push_back({"three conv layers, three noise GVPs", c, true, false});
        c = base_config(); c.pharm_nf = 16;
        cases.push_back({"pharm_nf 16 (no n16 tail stream)", c, true, false});
        cases.push_back({"128/16, spec and wide", base_config(), true, true});
        c = base_config(); c.n_hidden_scalars = 64; c.vector_size = 32;
        cases.push_back({"64/32 wide", c, false, true});
        c = base_config(); c.n_hidden_scalars = 256; c.vector_size = 32;
        cases.push_back({"256/32 wide", c, false, true});
        // feature counts at the ends of pf_create's range (tests/test_gpu_feature_counts.py runs them on the device)
        c = base_config(); c.pharm_nf = 1; c.rec_nf = 1;
        cases.push_back({"pharm_nf 1, rec_nf 1, spec and wide", c, true, true});
        c = base_config(); c.pharm_nf = 16; c.rec_nf = 40;
        cases.push_back({"pharm_nf 16, rec_nf 40, spec and wide", c, true, true});
    }
    for (size_t k = 0; k < cases.size(); ++k) {
        const Case& cs = cases[k];
        const int before = g_fail;
        const TensorList exp = expected_tensors(cs.c);
        RawMap raw;
        std::vector<float> flat;
        for (const auto& kv : exp) {
            RawTensor t;
            t.shape = kv.second;
            size_t numel = 1;
            for (int64_t d : kv.second) numel *= (size_t)d;
            for (size_t i = 0; i < numel; ++i) t.data.push_back(seeded((uint32_t)(k + 1), (uint32_t)(flat.size() + i)));
            flat.insert(flat.end(), t.data.begin(), t.data.end());
            raw[kv.first] = std::move(t);
        }
        PackedModel pm;
        std::string err;
        const int rc = pack_model(cs.c, raw, cs.spec, cs.wide, pm, err);
        CHECK(rc == PF_OK, "pack_model: %d (%s)", rc, err.c_str());
        if (rc == PF_OK) {
            check_values(cs, pm, flat, exp);
            check_layout(cs, pm);
            check_offsets(cs, exp);
            if (dump_dir) {
                const std::string b = std::string(dump_dir) + "/cfg" + std::to_string(k + 1);
                dump(b + ".w", pm.w.data(), pm.w.size() * sizeof(float));
                dump(b + ".map", pm.map.data(), pm.map.size() * sizeof(int));
                dump(b + ".split", pm.split_tab.data(), pm.split_tab.size() * sizeof(int4));
            }
        }
        printf("%s  config %zu (%s): %zu parameters -> %zu packed floats, %zu split words\n", g_fail == before ? "ok  " : "FAIL", k + 1, cs.name,
               flat.size(), pm.w.size(), pm.split_tab.size());
    }
    {   // the three validation messages
        const pf_config c = base_config();
        RawMap raw;
        for (const auto& kv : expected_tensors(c)) {
            RawTensor t; t.shape = kv.second; size_t numel = 1;
            for (int64_t d : kv.second) numel *= (size_t)d;
            t.data.assign(numel, 0.5f);
            raw[kv.first] = std::move(t);
        }
        PackedModel pm; std::string err;
        RawMap r1 = raw; r1.erase("dynamics.prot_encoder.0.bias");
        CHECK(pack_model(c, r1, true, false, pm, err) == PF_ERR_WEIGHT && err == "missing weight tensor dynamics.prot_encoder.0.bias", "missing: %s", err.c_str());
        RawMap r2 = raw; r2["dynamics.prot_encoder.0.bias"].shape = {127};
        CHECK(pack_model(c, r2, true, false, pm, err) == PF_ERR_WEIGHT && err == "wrong shape for dynamics.prot_encoder.0.bias", "shape: %s", err.c_str());
        RawMap r3 = raw; r3["extra.weight"] = RawTensor{{1}, {1.f}};
        CHECK(pack_model(c, r3, true, false, pm, err) == PF_ERR_WEIGHT && err == "unexpected weight tensor extra.weight", "unexpected: %s", err.c_str());
    }
    {   // a list that lacks a name the offsets table needs is rejected with a message, never answered with -1
        const pf_config c = base_config();
        TensorList cut = expected_tensors(c);
        cut.pop_back();                     // to_scalar_output.bias
        FlatLayout lay; ParamOffsets po; std::string err;
        CHECK(param_offsets(c, cut, lay, po, err) == PF_ERR_STATE &&
              err == "internal: parameter dynamics.noise_predictor.noise_predictor.to_scalar_output.bias is not in the flat layout", "truncated list: %s", err.c_str());
        cut = expected_tensors(c);
        cut.erase(cut.begin() + 9);         // the first message GVP's Wu
        CHECK(param_offsets(c, cut, lay, po, err) == PF_ERR_STATE && err.find("edge_message_fns.pharm_ff_pharm.0.Wu is not in the flat layout") != std::string::npos,
              "list without a GVP tensor: %s", err.c_str());
    }
    printf(g_fail ? "pack_check: %d check(s) FAILED\n" : "pack_check: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
