// bind_check -- the bind planner (csrc/pf_bind.cpp) on the CPU: plans seeded batches for a handful of configurations, fills
// their table section into a buffer of exactly table_total bytes and checks regions, tiles, the CSR, the three layouts, the
// share decision, the one-hot verdict and every rejection -- each restated here, independently of the planner's code.
// Built and run by tests/test_bind_host.py (host only, under the address and undefined-behaviour sanitizers).
// Exit status 0: every check held.
// Left out: "edge capacity too large" (more than 2^31 / 128 edge slots: a batch far too big for a unit test).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "pf_bind.h"

using namespace pfbind;

static int g_fail = 0;
// the planner's 8-edge pass is compiled for AVX2; whether the CPU has it is the caller's to find out (pf_host.cpp does the same).
// Without it the "on" legs below run the scalar pass twice
#if defined(__x86_64__)
static const bool g_have_avx2 = __builtin_cpu_supports("avx2");
#else
static const bool g_have_avx2 = false;
#endif
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            if (++g_fail <= 30) { printf("  FAIL: "); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                     \
    } while (0)

// value i of the seeded stream: a 32-bit integer hash (lowbias32) of the counter
static uint32_t hash32(uint32_t seed, uint32_t i) {
    uint32_t x = i + seed * 0x9E3779B9u;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
static float seeded(uint32_t seed, uint32_t i) { return (float)(hash32(seed, i) >> 8) * (1.0f / 16777216.0f); }     // [0, 1)

struct Batch {
    std::vector<int> prot_ptr{0}, pharm_ptr{0}, src, dst;
    std::vector<float> x, h;
    int rec_nf = 11;
    int B() const { return (int)prot_ptr.size() - 1; }
    int Np() const { return prot_ptr.back(); }
    int Nf() const { return pharm_ptr.back(); }
    // a graph of np seeded atoms in a cube of edge `box`; its pp edges by brute force within `cutoff`,
    // grouped by destination, ascending.  The same seed and size give the same pocket: a copy
    void add(uint32_t seed, int np, int nf, float cutoff = 3.5f, float box = 9.0f) {
        const int p0 = Np();
        for (int i = 0; i < np; ++i) {
            for (int k = 0; k < 3; ++k) x.push_back(box * seeded(seed, 3 * i + k));
            const int ty = (int)(hash32(seed + 77, i) % (uint32_t)rec_nf);
            for (int k = 0; k < rec_nf; ++k) h.push_back(k == ty ? 1.0f : 0.0f);
        }
        for (int d = 0; d < np; ++d)
            for (int s = 0; s < np; ++s) {
                if (s == d) continue;
                float r2 = 0;
                for (int k = 0; k < 3; ++k) { const float u = x[(size_t)(p0 + s) * 3 + k] - x[(size_t)(p0 + d) * 3 + k]; r2 += u * u; }
                if (r2 < cutoff * cutoff) { src.push_back(p0 + s); dst.push_back(p0 + d); }
            }
        prot_ptr.push_back(p0 + np);
        pharm_ptr.push_back(Nf() + nf);
    }
};

struct Case { const char* name; pf_config c; bool spec, wide; };

static pf_config base_config() {
    pf_config c{};
    c.abi_version = PF_ABI_VERSION;
    c.pharm_nf = 6; c.rec_nf = 11; c.vector_size = 16; c.n_hidden_scalars = 128;
    c.n_convs = 2; c.n_message_gvps = 3; c.n_update_gvps = 2; c.n_noise_gvps = 4;
    c.rbf_dim = 16;
    c.message_norm_mode = PF_NORM_MEAN;
    c.ff_k = 0; c.pf_k = 5;
    return c;
}

static BindInputs inputs_of(const Case& cs, const Batch& b, bool host_rows, bool avx2, const std::vector<int>& rep = {}) {
    BindInputs in;
    in.cfg = cs.c; in.B = b.B(); in.prot_ptr = b.prot_ptr.data(); in.pharm_ptr = b.pharm_ptr.data();
    in.n_pp = (int64_t)b.src.size(); in.pp_src = b.src.data(); in.pp_dst = b.dst.data();
    in.host_rows = host_rows; in.host_prot_x = host_rows ? b.x.data() : nullptr; in.host_prot_h = host_rows ? b.h.data() : nullptr;
    in.rep = rep;
    in.spec = cs.spec; in.wide = cs.wide; in.pa_check = false; in.edge_rec = 1; in.n16_rows_max = 24000;
    in.allow_avx2 = avx2 && g_have_avx2;
    return in;
}

// the table section as fill_tables leaves it, in a buffer of exactly table_total bytes (the sanitizer sees any overrun); what lies
// behind table_bytes (the pocket rows of a device-resident batch) must stay untouched
struct Tables {
    BindPlan p; FillResult fr; std::vector<unsigned char> bytes; int rc = PF_OK; std::string msg;
};
static Tables run(const BindInputs& in) {
    Tables t;
    BindError err;
    t.rc = plan_batch(in, t.p, err);
    if (t.rc) { t.msg = err.msg; return t; }
    unsigned char* buf = static_cast<unsigned char*>(malloc(t.p.table_total));
    memset(buf, 0xA5, t.p.table_total);
    t.rc = fill_tables(t.p, in, buf, t.fr, err);
    t.msg = err.msg;
    for (size_t i = t.p.table_bytes; i < t.p.table_total; ++i)
        if (buf[i] != 0xA5) { CHECK(false, "fill_tables wrote byte %zu, behind table_bytes %zu", i, t.p.table_bytes); break; }
    t.bytes.assign(buf, buf + t.p.table_total);
    free(buf);
    return t;
}
template <typename T>
static const T* tab(const Tables& t, size_t off) { return reinterpret_cast<const T*>(t.bytes.data() + off); }

// the meaningful bytes of two table sections agree (padding between buffers is never written)
static bool same_tables(const Tables& a, const Tables& b) {
    const BindPlan &p = a.p, &q = b.p;
    if (memcmp(&p.t, &q.t, sizeof(TableOff)) || memcmp(&p.z, &q.z, sizeof(ZeroOff)) || memcmp(&p.s, &q.s, sizeof(ScratchOff))) return false;
    if (p.table_bytes != q.table_bytes || p.table_total != q.table_total || p.ws_bytes != q.ws_bytes || p.zero_bytes != q.zero_bytes) return false;
    if (p.Ecap != q.Ecap || p.h_reg != q.h_reg || p.h_cap != q.h_cap || p.deg != q.deg || p.epp_g != q.epp_g || p.maxdeg != q.maxdeg ||
        p.pfq != q.pfq || p.reg_act != q.reg_act || p.cap_act != q.cap_act || p.gid != q.gid) return false;
    if (a.fr.share != b.fr.share || a.fr.share_rows != b.fr.share_rows || a.fr.h_share_start != b.fr.h_share_start ||
        a.fr.h_share_cnt != b.fr.h_share_cnt || a.fr.host_onehot != b.fr.host_onehot) return false;
    const size_t E = (size_t)std::max<int64_t>(p.Ecap, 1), N = (size_t)p.N, B = (size_t)p.B;
    struct { size_t off, n; } span[] = {
        {p.t.pptr, (B + 1) * 4}, {p.t.fptr, (B + 1) * 4}, {p.t.gid, N * 4}, {p.t.reg, 16 * B}, {p.t.regact, 4 * B},
        {p.t.eta, p.et_act.size() * sizeof(EdgeTile)}, {p.t.nta, p.n_act.size() * sizeof(NodeTile)}, {p.t.esrc, E * 4}, {p.t.edst, E * 4},
        {p.t.ins, 16 * N}, {p.t.inc, 16 * N}, {p.t.ppc, 4 * B}, {p.t.et, p.et_tiles.size() * sizeof(EdgeTile)},
        {p.t.nt, p.n_tiles.size() * sizeof(NodeTile)}, {p.t.ht, p.h_tiles.size() * sizeof(NodeTile)}, {p.t.pfq, p.pfq.empty() ? 0 : 4 * B},
        {p.t.regs, 16 * B}, {p.t.pas, 4 * B}, {p.t.repb, 4 * B}};
    for (const auto& s : span)
        if (s.n && memcmp(a.bytes.data() + s.off, b.bytes.data() + s.off, s.n)) return false;
    return true;
}

static int active_ref(const pf_config& c, int np, int nf) {      // the active atoms of a graph
    if (c.pf_k > 0) return std::min(np, nf * std::min(c.pf_k, np));
    return nf > 0 ? np : 0;
}

// everything a successful bind must satisfy
static void check_tables(const Case& cs, const Batch& b, const BindInputs& in, const Tables& t, const char* what) {
    const int f0 = g_fail;
    const pf_config& c = cs.c;
    const BindPlan& p = t.p;
    const int B = b.B(), Np = b.Np(), Nf = b.Nf(), N = Np + Nf;
    const int64_t n_pp = (int64_t)b.src.size();
    CHECK(p.B == B && p.Np == Np && p.Nf == Nf && p.N == N && p.n_pp == n_pp, "%s: sizes", what);
    // ---- the reference CSR: a stable sort of the input by destination
    std::vector<int> order(n_pp);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int bb) { return b.dst[a] < b.dst[bb]; });
    std::vector<int> indeg(Np, 0), first(Np + 1, 0), epp(B, 0), maxdeg(B, 0), graph_of(N, 0);
    for (int g = 0; g < B; ++g) {
        for (int i = b.prot_ptr[g]; i < b.prot_ptr[g + 1]; ++i) graph_of[i] = g;
        for (int i = b.pharm_ptr[g]; i < b.pharm_ptr[g + 1]; ++i) graph_of[Np + i] = g;
    }
    for (int64_t e = 0; e < n_pp; ++e) indeg[b.dst[e]]++;
    for (int i = 0; i < Np; ++i) {
        first[i + 1] = first[i] + indeg[i];
        epp[graph_of[i]] += indeg[i];
        maxdeg[graph_of[i]] = std::max(maxdeg[graph_of[i]], indeg[i]);
    }
    int mnp = 0, mnf = 0;
    for (int g = 0; g < B; ++g) { mnp = std::max(mnp, b.prot_ptr[g + 1] - b.prot_ptr[g]); mnf = std::max(mnf, b.pharm_ptr[g + 1] - b.pharm_ptr[g]); }
    CHECK(p.max_np == mnp && p.max_nf == mnf, "%s: max_np %d / max_nf %d, expected %d / %d", what, p.max_np, p.max_nf, mnp, mnf);
    // ---- regions: at or after n_pp, 32-aligned, ascending, disjoint, capacities by the formulas of DESIGN section 3
    int64_t end = n_pp;
    int act_total = 0;
    CHECK(p.h_reg.size() == (size_t)4 * B && p.h_cap.size() == (size_t)4 * B, "%s: h_reg / h_cap are not [4][B]", what);
    for (int et = 0; et < 4; ++et)
        for (int g = 0; g < B; ++g) {
            const int np = b.prot_ptr[g + 1] - b.prot_ptr[g], nf = b.pharm_ptr[g + 1] - b.pharm_ptr[g];
            int cap;
            if (et == 0) cap = nf * (c.ff_k > 0 ? std::min(c.ff_k, std::max(nf - 1, 0)) : std::max(nf - 1, 0));
            else if (et == 1 || et == 2) cap = nf * (c.pf_k > 0 ? std::min(c.pf_k, np) : np);
            else {
                const int nact = active_ref(c, np, nf);
                cap = (int)std::min<int64_t>(epp[g], (int64_t)nact * maxdeg[g]);
                CHECK(p.reg_act[g] == act_total && p.cap_act[g] == nact, "%s: active list of graph %d at %d + %d, expected %d + %d", what, g,
                      p.reg_act[g], p.cap_act[g], act_total, nact);
                act_total += nact;
            }
            const int reg = p.h_reg[(size_t)et * B + g];
            CHECK(reg >= end && reg % 32 == 0 && reg < end + 32, "%s: region (%d, %d) starts at %d, the previous one ends at %lld", what, et, g, reg, (long long)end);
            CHECK(p.h_cap[(size_t)et * B + g] == cap, "%s: region (%d, %d) holds %d slots, expected %d", what, et, g, p.h_cap[(size_t)et * B + g], cap);
            end = (int64_t)reg + cap;
        }
    CHECK(p.Ecap == end, "%s: Ecap %lld, the last region ends at %lld", what, (long long)p.Ecap, (long long)end);
    CHECK(p.act_total == act_total, "%s: act_total %d, expected %d", what, p.act_total, act_total);
    const int64_t E = std::max<int64_t>(p.Ecap, 1);
    // ---- tiles: each list covers each of its regions exactly once, 1..32 slots per tile, in etype order
    auto region_tiles = [&](const std::vector<EdgeTile>& tiles, const int* t0, int n_et, const char* list) {
        size_t k = 0;
        for (int et = 0; et < n_et; ++et) {
            CHECK(t0[et] == (int)k, "%s: %s etype %d starts at tile %d, expected %zu", what, list, et, t0[et], k);
            for (int g = 0; g < B; ++g) {
                const int cap = p.h_cap[(size_t)et * B + g], reg = p.h_reg[(size_t)et * B + g];
                for (int o = 0; o < cap; o += 32, ++k) {
                    if (k >= tiles.size()) { CHECK(false, "%s: %s ends early", what, list); return k; }
                    const EdgeTile& x = tiles[k];
                    CHECK(x.e0 == reg + o && x.n == std::min(32, cap - o) && x.n >= 1 && x.n <= 32 && x.et == (et == 3 ? (int)ET_PP : et) &&
                          x.cnt_idx == et * B + g && x.rel == o, "%s: %s tile %zu", what, list, k);
                }
            }
        }
        return k;
    };
    {
        size_t k = region_tiles(p.et_tiles, p.et_tile0, 3, "et_tiles");
        CHECK(p.et_tile0[3] == (int)k, "%s: pp tiles start at %d, expected %zu", what, p.et_tile0[3], k);
        CHECK(p.n_edge_tiles_last == p.et_tile0[2], "%s: n_edge_tiles_last %d does not end the pf tiles (%d)", what, p.n_edge_tiles_last, p.et_tile0[2]);
        for (int64_t o = 0; o < n_pp; o += 32, ++k) {
            if (k >= p.et_tiles.size()) { CHECK(false, "%s: the pp tiles end early", what); break; }
            const EdgeTile& x = p.et_tiles[k];
            CHECK(x.e0 == o && x.n == std::min<int64_t>(32, n_pp - o) && x.et == ET_PP && x.cnt_idx == -1 && x.rel == 0, "%s: pp tile %zu", what, k);
        }
        CHECK(k == p.et_tiles.size() && p.et_tile0[4] == (int)k && p.n_edge_tiles == (int)k, "%s: %zu edge tiles, expected %zu", what, p.et_tiles.size(), k);
        k = region_tiles(p.et_act, p.et_tile0_act, 4, "et_act");
        CHECK(k == p.et_act.size() && p.et_tile0_act[4] == (int)k && p.n_edge_tiles_act == (int)k, "%s: %zu pruned edge tiles, expected %zu", what, p.et_act.size(), k);
    }
    {   // node tiles: centers [Np, N) first, then atoms [0, Np); head tiles = the center tiles; the act list: center tiles + cap_act
        size_t k = 0;
        auto expect = [&](const std::vector<NodeTile>& v, size_t i, int n0, int n, int ntype, int cnt_idx, int rel, int ids, const char* list) {
            if (i >= v.size()) { CHECK(false, "%s: %s ends early", what, list); return; }
            const NodeTile& x = v[i];
            CHECK(x.n0 == n0 && x.n == n && n >= 1 && n <= 32 && x.ntype == ntype && x.cnt_idx == cnt_idx && x.rel == rel && x.ids == ids, "%s: %s tile %zu", what, list, i);
        };
        for (int o = 0; o < Nf; o += 32, ++k) {
            expect(p.n_tiles, k, Np + o, std::min(32, Nf - o), 1, -1, 0, 0, "n_tiles");
            expect(p.h_tiles, k, Np + o, std::min(32, Nf - o), 1, -1, 0, 0, "h_tiles");
            expect(p.n_act, k, Np + o, std::min(32, Nf - o), 1, -1, 0, 0, "n_act");
        }
        const size_t nh = k;
        CHECK(p.h_tiles.size() == nh && p.n_head_tiles == (int)nh && p.n_node_tiles_last == (int)nh, "%s: %zu head tiles, expected %zu", what, p.h_tiles.size(), nh);
        for (int o = 0; o < Np; o += 32, ++k) expect(p.n_tiles, k, o, std::min(32, Np - o), 0, -1, 0, 0, "n_tiles");
        CHECK(p.n_tiles.size() == k && p.n_node_tiles == (int)k, "%s: %zu node tiles, expected %zu", what, p.n_tiles.size(), k);
        k = nh;
        for (int g = 0; g < B; ++g)
            for (int o = 0; o < p.cap_act[g]; o += 32, ++k) expect(p.n_act, k, p.reg_act[g] + o, std::min(32, p.cap_act[g] - o), 0, 4 * B + g, o, 1, "n_act");
        CHECK(p.n_act.size() == k && p.n_node_tiles_act == (int)k, "%s: %zu pruned node tiles, expected %zu", what, p.n_act.size(), k);
    }
    // ---- layouts: 256-aligned, inside their section, no overlap (sizes restated)
    {
        const size_t S = (size_t)c.n_hidden_scalars, V3 = (size_t)3 * c.vector_size;
        auto so = [&](size_t bytes) { return cs.spec ? bytes : (size_t)16; };
        struct Buf { const char* name; size_t off, bytes; };
        const TableOff& o = p.t;
        const std::vector<Buf> tabs = {
            {"pptr", o.pptr, (size_t)(B + 1) * 4}, {"fptr", o.fptr, (size_t)(B + 1) * 4}, {"gid", o.gid, (size_t)N * 4}, {"reg", o.reg, (size_t)16 * B},
            {"regact", o.regact, (size_t)4 * B}, {"eta", o.eta, p.et_act.size() * sizeof(EdgeTile)}, {"nta", o.nta, p.n_act.size() * sizeof(NodeTile)},
            {"esrc", o.esrc, (size_t)E * 4}, {"edst", o.edst, (size_t)E * 4}, {"ins", o.ins, (size_t)16 * N}, {"inc", o.inc, (size_t)16 * N},
            {"ppc", o.ppc, (size_t)4 * B}, {"et", o.et, p.et_tiles.size() * sizeof(EdgeTile)}, {"nt", o.nt, p.n_tiles.size() * sizeof(NodeTile)},
            {"ht", o.ht, p.h_tiles.size() * sizeof(NodeTile)}, {"pfq", o.pfq, (size_t)4 * B}, {"regs", o.regs, (size_t)16 * B}, {"pas", o.pas, (size_t)4 * B},
            {"repb", o.repb, (size_t)4 * B}};
        const std::vector<Buf> rows = {{"px0", o.px0, (size_t)Np * 12}, {"ph0", o.ph0, (size_t)Np * c.rec_nf * 4}};
        const ZeroOff& z = p.z;
        const std::vector<Buf> zero = {
            {"dyn", z.dyn, (size_t)20 * B}, {"act", z.act, (size_t)(act_total + 1) * 4}, {"flag", z.flag, 256}, {"gnorm", z.gnorm, (size_t)8 * B},
            {"need", z.need, (size_t)std::max(Np, 1) * 4}, {"lpart", z.lpart, 64 + (size_t)((Nf + 63) / 64) * 32}, {"pastamp", z.pastamp, (size_t)std::max(Np, 1) * 4},
            {"pasame", z.pasame, (size_t)4 * B}, {"pacnt", z.pacnt, (size_t)(B + 1) * 4}, {"pagst", z.pagst, in.pa_check ? (size_t)(E / 16 + 1) * 4 : 16}};
        const ScratchOff& s = p.s;
        const size_t Nf1 = (size_t)std::max(Nf, 1), Np1 = (size_t)std::max(Np, 1);
        const std::vector<Buf> scratch = {
            {"xn", s.xn, (size_t)N * 16}, {"fh", s.fh, (size_t)Nf * c.pharm_nf * 4}, {"t", s.t, (size_t)4 * B}, {"h0", s.h0, N * S * 4}, {"h1", s.h1, N * S * 4},
            {"v0", s.v0, N * V3 * 4}, {"v1", s.v1, N * V3 * 4}, {"ms", s.ms, (size_t)(E + 1) * S * 4}, {"mv", s.mv, (size_t)(E + 1) * V3 * 4},
            {"ms2", s.ms2, p.msg2 ? (size_t)(E + 1) * 128 * 4 : 16}, {"mv2", s.mv2, p.msg2 ? (size_t)(E + 1) * 48 * 4 : 16},
            {"eh", s.eh, (size_t)Nf * c.pharm_nf * 4}, {"ex", s.ex, (size_t)Nf * 12}, {"c0", s.c0, (size_t)12 * B}, {"c1", s.c1, (size_t)12 * B},
            {"pre", s.pre, so(Np1 * 128 * 4)}, {"eorig", s.eorig, (size_t)E * 4}, {"ptype", s.ptype, Np1 * 4},
            {"rec", s.rec, (size_t)(in.edge_rec ? 3 * p.rec_slots : 0) * 16}, {"zs", s.zs, so((size_t)std::max<int64_t>(n_pp, 1) * 128 * 4)},
            {"ptpg", s.ptpg, so((size_t)B * 4 * c.rec_nf * 128 * 4)}, {"xchg", s.xchg, 2 * Nf1 * 20 * 4}, {"cenh", s.cenh, so(Nf1 * 128 * 4)},
            {"cenp", s.cenp, so(2 * Nf1 * 128 * 4)}, {"snap", s.snap, 2 * (Nf1 * c.pharm_nf + 4) * 4}};
        auto section = [&](const std::vector<Buf>& v, size_t begin, size_t limit, const char* sec) {
            size_t prev_end = begin;
            for (const Buf& x : v) {
                CHECK(x.off % 256 == 0, "%s: %s.%s at %zu is not 256-aligned", what, sec, x.name, x.off);
                CHECK(x.off >= prev_end, "%s: %s.%s at %zu overlaps the buffer before it (ends at %zu)", what, sec, x.name, x.off, prev_end);
                CHECK(x.off + x.bytes <= limit, "%s: %s.%s [%zu, %zu) leaves its section (%zu)", what, sec, x.name, x.off, x.off + x.bytes, limit);
                prev_end = x.off + x.bytes;
            }
        };
        section(tabs, 0, p.index_bytes, "table");
        section(rows, p.index_bytes, p.table_total, "table");
        section(zero, 0, p.zero_bytes, "zero");
        section(scratch, p.zero_bytes, p.ws_bytes, "scratch");
        CHECK(p.index_bytes % 256 == 0 && p.zero_bytes % 256 == 0 && p.table_total % 256 == 0 && p.ws_bytes % 256 == 0, "%s: section sizes", what);
        CHECK(p.table_bytes == (in.host_rows ? p.table_total : p.index_bytes), "%s: table_bytes %zu (index %zu, total %zu)", what, p.table_bytes, p.index_bytes, p.table_total);
        CHECK(p.rec_slots == (B <= 64 ? E : 0), "%s: rec_slots", what);
        CHECK(p.msg2 == (!cs.wide && c.n_convs == 2 && (long)p.n_edge_tiles_act * 32 <= in.n16_rows_max), "%s: msg2", what);
    }
    // ---- pfq: center j's min(k, Np_g) edges on the graph that owns protein atom j
    if (c.message_norm_mode == PF_NORM_GRAPH && c.pf_k > 0) {
        std::vector<int> q(B, 0);
        for (int g = 0; g < B; ++g)
            for (int j = b.pharm_ptr[g]; j < b.pharm_ptr[g + 1]; ++j) {
                const int k = std::min(c.pf_k, b.prot_ptr[g + 1] - b.prot_ptr[g]);
                if (k > 0) q[graph_of[j]] += k;
            }
        CHECK(p.pfq == q, "%s: pfq", what);
        CHECK(!memcmp(tab<int>(t, p.t.pfq), q.data(), (size_t)4 * B), "%s: the pfq table", what);
    } else CHECK(p.pfq.empty(), "%s: pfq without graph norm", what);
    // ---- CSR and the small tables
    const int *esrc = tab<int>(t, p.t.esrc), *edst = tab<int>(t, p.t.edst), *ins = tab<int>(t, p.t.ins), *inc = tab<int>(t, p.t.inc);
    for (int64_t e = 0; e < n_pp; ++e)
        if (esrc[e] != b.src[order[e]] || edst[e] != b.dst[order[e]]) { CHECK(false, "%s: CSR edge %lld", what, (long long)e); break; }
    for (int64_t e = n_pp; e < E; ++e)
        if (esrc[e] || edst[e]) { CHECK(false, "%s: slot %lld beyond n_pp is not zero", what, (long long)e); break; }
    const bool share = t.fr.share;
    std::vector<int> rep_first(Np, 0), rep_cnt(Np, 0);
    if (share)
        for (int g = 0; g < B; ++g)
            for (int i = 0; i < b.prot_ptr[g + 1] - b.prot_ptr[g]; ++i) {
                rep_first[b.prot_ptr[g] + i] = first[b.prot_ptr[in.rep[g]] + i];
                rep_cnt[b.prot_ptr[g] + i] = indeg[b.prot_ptr[in.rep[g]] + i];
            }
    for (int slot = 0; slot < 4; ++slot)
        for (int i = 0; i < N; ++i) {
            int es = 0, ec = 0;
            if (slot == 1 && i < Np) { es = first[i]; ec = indeg[i]; }
            if (slot == 3 && i < Np) { es = rep_first[i]; ec = rep_cnt[i]; }
            if (ins[(size_t)slot * N + i] != es || inc[(size_t)slot * N + i] != ec) { CHECK(false, "%s: in-edge range slot %d node %d", what, slot, i); slot = 4; break; }
        }
    const int *ppc = tab<int>(t, p.t.ppc), *regs = tab<int>(t, p.t.regs), *pas = tab<int>(t, p.t.pas), *repb = tab<int>(t, p.t.repb);
    long share_rows = 0;
    for (int g = 0; g < B; ++g) {
        CHECK(ppc[g] == epp[g], "%s: pp_cnt[%d] %d, expected %d", what, g, ppc[g], epp[g]);
        const bool is_rep = share && in.rep[g] == g;
        CHECK(pas[g] == (is_rep ? epp[g] : 0), "%s: pa_static[%d]", what, g);
        CHECK(repb[g] == (share ? b.prot_ptr[in.rep[g]] : 0), "%s: rep_base[%d]", what, g);
        for (int et = 0; et < 4; ++et) {
            const int want = (share && et == 3) ? (is_rep ? first[b.prot_ptr[g]] : 0) : p.h_reg[(size_t)et * B + g];
            CHECK(regs[(size_t)et * B + g] == want, "%s: regs[%d][%d] %d, expected %d", what, et, g, regs[(size_t)et * B + g], want);
            if (et < 3) share_rows += p.h_cap[(size_t)et * B + g];
        }
        CHECK(t.fr.h_share_start[g] == (is_rep ? first[b.prot_ptr[g]] : 0) && t.fr.h_share_cnt[g] == (is_rep ? epp[g] : 0), "%s: h_share[%d]", what, g);
        if (is_rep) share_rows += epp[g];
    }
    CHECK(t.fr.share_rows == (share ? share_rows : 0), "%s: share_rows %ld, expected %ld", what, t.fr.share_rows, share ? share_rows : 0);
    CHECK(!memcmp(tab<int>(t, p.t.pptr), b.prot_ptr.data(), (size_t)(B + 1) * 4) && !memcmp(tab<int>(t, p.t.fptr), b.pharm_ptr.data(), (size_t)(B + 1) * 4), "%s: ptr tables", what);
    CHECK(N == 0 || !memcmp(tab<int>(t, p.t.gid), graph_of.data(), (size_t)N * 4), "%s: gid table", what);
    CHECK(!memcmp(tab<int>(t, p.t.reg), p.h_reg.data(), (size_t)16 * B) && !memcmp(tab<int>(t, p.t.regact), p.reg_act.data(), (size_t)4 * B), "%s: region tables", what);
    auto same = [&](size_t off, const void* v, size_t n) { return n == 0 || !memcmp(t.bytes.data() + off, v, n); };
    CHECK(same(p.t.eta, p.et_act.data(), p.et_act.size() * sizeof(EdgeTile)) && same(p.t.nta, p.n_act.data(), p.n_act.size() * sizeof(NodeTile)) &&
          same(p.t.et, p.et_tiles.data(), p.et_tiles.size() * sizeof(EdgeTile)) && same(p.t.nt, p.n_tiles.data(), p.n_tiles.size() * sizeof(NodeTile)) &&
          same(p.t.ht, p.h_tiles.data(), p.h_tiles.size() * sizeof(NodeTile)), "%s: tile tables", what);
    if (in.host_rows) {
        CHECK(same(p.t.px0, b.x.data(), (size_t)Np * 12) && same(p.t.ph0, b.h.data(), (size_t)Np * c.rec_nf * 4), "%s: pocket rows", what);
        CHECK(t.fr.host_onehot == (Np > 0 ? 1 : 0), "%s: one-hot verdict %d of one-hot rows", what, t.fr.host_onehot);
    } else CHECK(t.fr.host_onehot == -1, "%s: one-hot verdict of device rows", what);
    if (g_fail != f0) printf("  (%s: %d checks failed)\n", what, g_fail - f0);
}

static Batch ragged_five() {
    Batch b;
    const int np[5] = {48, 300, 40, 64, 32}, nf[5] = {3, 8, 5, 1, 6};
    for (int g = 0; g < 5; ++g) b.add(200 + g, np[g], nf[g], 3.5f, g == 1 ? 14.0f : 9.0f);
    return b;
}

static void expect_reject(const Case& cs, const Batch& b, const std::vector<int>& rep, bool host_rows, const char* phrase, bool plan_phase) {
    for (int avx2 = 0; avx2 < 2; ++avx2) {
        const BindInputs in = inputs_of(cs, b, host_rows, avx2 != 0, rep);
        BindPlan p;
        p.B = -77; p.Ecap = 12345; p.ws_bytes = 99;              // a failing plan leaves its output as it was
        BindError err;
        int rc = plan_batch(in, p, err);
        if (plan_phase) {
            CHECK(rc == PF_ERR_ARG && err.msg.find(phrase) != std::string::npos, "rejection \"%s\": plan_batch gave %d \"%s\"", phrase, rc, err.msg.c_str());
            CHECK(!err.batch_lost, "rejection \"%s\" must leave the previous batch intact", phrase);
            CHECK(p.B == -77 && p.Ecap == 12345 && p.ws_bytes == 99 && p.gid.empty() && p.deg.empty() && p.h_reg.empty() && p.et_tiles.empty(),
                  "rejection \"%s\" touched the output plan", phrase);
            continue;
        }
        CHECK(rc == PF_OK, "rejection \"%s\": the plan itself failed with \"%s\"", phrase, err.msg.c_str());
        if (rc) continue;
        std::vector<unsigned char> buf(p.table_total);
        FillResult fr;
        rc = fill_tables(p, in, buf.data(), fr, err);
        CHECK(rc == PF_ERR_ARG && err.msg.find(phrase) != std::string::npos, "rejection \"%s\": fill_tables gave %d \"%s\"", phrase, rc, err.msg.c_str());
    }
}

int main() {
    if (!g_have_avx2) printf("(no AVX2 on this CPU: the AVX2 legs are skipped, both passes are the scalar one)\n");
    std::vector<Case> cases;
    cases.push_back({"default", base_config(), true, false});
    { Case k{"pf_k0", base_config(), true, false}; k.c.pf_k = 0; cases.push_back(k); }
    { Case k{"ff_k3", base_config(), true, false}; k.c.ff_k = 3; cases.push_back(k); }
    { Case k{"graph_norm", base_config(), true, false}; k.c.message_norm_mode = PF_NORM_GRAPH; cases.push_back(k); }
    { Case k{"wide_64_32", base_config(), false, true}; k.c.n_hidden_scalars = 64; k.c.vector_size = 32; cases.push_back(k); }

    std::vector<std::pair<std::string, Batch>> batches;
    { Batch b; b.add(1, 40, 3); batches.push_back({"one graph", b}); }
    batches.push_back({"ragged five", ragged_five()});
    { Batch b; b.add(11, 48, 4); b.add(12, 40, 0); b.add(13, 0, 3); b.add(14, 36, 2); batches.push_back({"no centers / no atoms", b}); }
    { Batch b; b.add(21, 30, 3, 0.0f); b.add(22, 20, 2, 0.0f); batches.push_back({"n_pp = 0", b}); }
    {   // region capacities of exactly 0, 32 and 33: no centers or one center (ff) give 0; with fewer atoms than pf_k, pf and fp hold nf np = 8 x 4, 11 x 3
        Batch b; b.add(31, 40, 0); b.add(32, 4, 8); b.add(33, 3, 11); b.add(34, 40, 1); batches.push_back({"capacities 0 / 32 / 33", b});
    }
    for (const Case& cs : cases) {
        printf("%s\n", cs.name);
        for (const auto& nb : batches) {
            for (int host_rows = 0; host_rows < 2; ++host_rows) {
                const BindInputs in = inputs_of(cs, nb.second, host_rows != 0, true);
                const Tables t = run(in);
                const std::string what = std::string(cs.name) + " / " + nb.first + (host_rows ? " / host rows" : " / device rows");
                CHECK(t.rc == PF_OK, "%s: rejected with \"%s\"", what.c_str(), t.msg.c_str());
                if (t.rc == PF_OK) check_tables(cs, nb.second, in, t, what.c_str());
            }
        }
    }
    const Case& dflt = cases[0];
    {   // the capacities the batch above was built for
        BindPlan p; BindError err;
        const BindInputs in = inputs_of(dflt, batches[4].second, false, true);
        CHECK(plan_batch(in, p, err) == PF_OK, "capacities: %s", err.msg.c_str());
        const int B = 4;
        CHECK(p.h_cap[0 * B + 0] == 0 && p.h_cap[1 * B + 0] == 0 && p.h_cap[0 * B + 3] == 0, "capacity 0 missing");
        CHECK(p.h_cap[1 * B + 1] == 32 && p.h_cap[2 * B + 1] == 32, "capacity 32 missing (%d)", p.h_cap[1 * B + 1]);
        CHECK(p.h_cap[1 * B + 2] == 33 && p.h_cap[2 * B + 2] == 33, "capacity 33 missing (%d)", p.h_cap[1 * B + 2]);
    }
    {   // pa_check on: the per-group stamps are sized by Ecap
        BindInputs in = inputs_of(dflt, batches[1].second, true, true);
        in.pa_check = true;
        const Tables t = run(in);
        CHECK(t.rc == PF_OK, "pa_check: %s", t.msg.c_str());
        if (t.rc == PF_OK) check_tables(dflt, batches[1].second, in, t, "default / ragged five / pa_check");
    }
    // ---- shuffled edges: the same tables as the sorted list (every configuration, the ragged batch)
    printf("shuffled edges, AVX2 pass\n");
    for (const Case& cs : cases) {
        const Batch& b = batches[1].second;
        Batch sh = b;
        {   // the destinations in a seeded random order; the edges of one destination stay together and in their order (the counting
            // sort is stable, so the sorted list's order of sources comes back)
            std::vector<int> o(b.src.size());
            std::iota(o.begin(), o.end(), 0);
            std::stable_sort(o.begin(), o.end(), [&](int x, int y) { return hash32(99, (uint32_t)b.dst[x]) < hash32(99, (uint32_t)b.dst[y]); });
            for (size_t e = 0; e < o.size(); ++e) { sh.src[e] = b.src[o[e]]; sh.dst[e] = b.dst[o[e]]; }
        }
        CHECK(!std::is_sorted(sh.dst.begin(), sh.dst.end()), "the shuffle left the destinations sorted");
        const Tables a = run(inputs_of(cs, b, true, true)), s = run(inputs_of(cs, sh, true, true));
        CHECK(a.rc == PF_OK && s.rc == PF_OK, "%s: shuffled bind rejected", cs.name);
        CHECK(a.p.dst_sorted && !s.p.dst_sorted, "%s: dst_sorted %d / %d", cs.name, (int)a.p.dst_sorted, (int)s.p.dst_sorted);
        if (a.rc == PF_OK && s.rc == PF_OK) {
            CHECK(same_tables(a, s), "%s: a shuffled edge list gives other tables", cs.name);
            check_tables(cs, sh, inputs_of(cs, sh, true, true), s, "shuffled");
        }
        // ---- the AVX2 pass on and off: byte-identical
        const Tables off = run(inputs_of(cs, b, true, false));
        CHECK(off.rc == PF_OK && same_tables(a, off), "%s: the AVX2 pass changes the ragged batch's tables", cs.name);
    }
    for (int n : {1, 7, 8, 9, 16, 17}) {      // n_pp at and around the pass's 8-edge blocks: a chain 0 <- 1 <- 2 ... in one graph
        Batch b;
        b.add(40, 24, 3, 0.0f);
        for (int e = 0; e < n; ++e) { b.src.push_back(e + 1); b.dst.push_back(e / 2 + 2); }
        const Tables on = run(inputs_of(dflt, b, true, true)), off = run(inputs_of(dflt, b, true, false));
        CHECK(on.rc == PF_OK && off.rc == PF_OK && same_tables(on, off), "n_pp = %d: the AVX2 pass changes the tables", n);
        if (on.rc == PF_OK) check_tables(dflt, b, inputs_of(dflt, b, true, true), on, "n_pp sweep");
    }
    // ---- the share decision: two pockets with 3 and 2 copies (B = 5, nrep = 2: nrep * 4 > B, so dense * 4 <= percopy * 3 alone decides)
    printf("share decision\n");
    for (int pays = 0; pays < 2; ++pays) {
        Batch b;
        const int nf = pays ? 12 : 1;             // 12 centers x 5 neighbours activate every atom of a 40-atom pocket; one center activates 5
        for (int k = 0; k < 3; ++k) b.add(51, 40, nf);
        for (int k = 0; k < 2; ++k) b.add(52, 36, nf);
        const std::vector<int> rep = {0, 0, 0, 3, 3};
        std::vector<int> epp(5, 0);
        for (int d : b.dst) for (int g = 0; g < 5; ++g) if (d >= b.prot_ptr[g] && d < b.prot_ptr[g + 1]) epp[g]++;
        long dense = epp[0] + epp[3], percopy = 0;
        for (int g = 0; g < 5; ++g) {
            const int np = b.prot_ptr[g + 1] - b.prot_ptr[g];
            percopy += (long)(0.6 * active_ref(dflt.c, np, nf) * (double)epp[g] / np);
        }
        CHECK((dense * 4 <= percopy * 3) == (pays != 0), "share case %d: dense %ld, per-copy %ld do not decide as intended", pays, dense, percopy);
        CHECK(2 * 4 > 5, "nrep * 4 > B");
        for (int host_rows = 0; host_rows < 2; ++host_rows) {
            const BindInputs in = inputs_of(dflt, b, host_rows != 0, true, rep);
            const Tables t = run(in);
            CHECK(t.rc == PF_OK, "share case %d: %s", pays, t.msg.c_str());
            if (t.rc) continue;
            CHECK(t.fr.share == (pays != 0), "share case %d: share = %d (dense %ld, per-copy %ld)", pays, (int)t.fr.share, dense, percopy);
            check_tables(dflt, b, in, t, pays ? "sharing pays" : "sharing does not pay");
        }
    }
    // ---- the one-hot verdict
    {
        Batch b = batches[0].second;
        Tables t = run(inputs_of(dflt, b, true, true));
        CHECK(t.rc == PF_OK && t.fr.host_onehot == 1, "one-hot rows: verdict %d", t.fr.host_onehot);
        Batch two = b;
        two.h[(size_t)7 * two.rec_nf + 0] = 1.0f; two.h[(size_t)7 * two.rec_nf + 1] = 1.0f;
        t = run(inputs_of(dflt, two, true, true));
        CHECK(t.rc == PF_OK && t.fr.host_onehot == 0, "a row with two ones: verdict %d", t.fr.host_onehot);
        Batch half = b;
        for (int k = 0; k < half.rec_nf; ++k) if (half.h[(size_t)9 * half.rec_nf + k] == 1.0f) half.h[(size_t)9 * half.rec_nf + k] = 0.5f;
        t = run(inputs_of(dflt, half, true, true));
        CHECK(t.rc == PF_OK && t.fr.host_onehot == 0, "a row with 0.5: verdict %d", t.fr.host_onehot);
    }
    // ---- rejections
    printf("rejections\n");
    {
        const Batch good = ragged_five();
        { Batch b = good; b.prot_ptr[0] = 1; expect_reject(dflt, b, {}, false, "must start at 0", true); }
        { Batch b = good; b.pharm_ptr[0] = 1; expect_reject(dflt, b, {}, false, "must start at 0", true); }
        { Batch b = good; b.pharm_ptr[2] = b.pharm_ptr[1] - 1; expect_reject(dflt, b, {}, false, "non-decreasing", true); }
        { Batch b; b.add(60, 40, PF_MAXF + 1); expect_reject(dflt, b, {}, false, "pharmacophore centers (limit", true); }
        { Batch b = good; b.src[5] = -1; expect_reject(dflt, b, {}, false, "out of range", true); }
        { Batch b = good; b.dst.back() = b.Np(); expect_reject(dflt, b, {}, false, "out of range", true); }
        { Batch b = good; b.src[0] = b.prot_ptr[1] + 1; expect_reject(dflt, b, {}, false, "crosses graphs", true); }
        expect_reject(dflt, good, {0, 1, 2}, false, "named", true);
        {   // graph norm with kNN: a center index that the reference would look up behind the protein batch vector
            Batch b; b.add(61, 4, 3); b.add(62, 3, 6);       // 7 atoms, 9 centers
            expect_reject(cases[3], b, {}, false, "center index", true);
        }
        // false claims (after the point of no return): copies of one pocket ...
        Batch cp;
        for (int k = 0; k < 3; ++k) cp.add(70, 40, 3 + k);
        cp.add(71, 40, 4);                                   // another pocket with the same number of atoms
        cp.add(72, 36, 4);
        expect_reject(dflt, cp, {0, 0, 0, 3, 3}, false, "atoms,", false);
        expect_reject(dflt, cp, {0, 0, 1, 3, 4}, false, "not a representative", false);
        expect_reject(dflt, cp, {0, 0, 7, 3, 4}, false, "not a representative", false);
        {   // same atoms and edge count, one in-degree moved: the last edge into atom a goes into atom a2 of the same copy instead
            Batch b = cp;
            const int p1 = b.prot_ptr[1];
            size_t e = 0;
            while (e < b.dst.size() && b.dst[e] != p1 + 1) ++e;      // the first edge into atom 1 of graph 1 ... becomes the last into atom 0
            CHECK(e < b.dst.size(), "test setup: atom 1 of the copy has no in-edge");
            if (e == b.dst.size()) return 1;
            b.dst[e] = p1;
            if (b.src[e] == p1) b.src[e] = p1 + 2;
            expect_reject(dflt, b, {0, 0, 0, 3, 4}, false, "pp in-degree of atom", false);
        }
        {   // same in-degrees, one source redirected inside the graph
            Batch b = cp;
            const int p1 = b.prot_ptr[1];
            size_t e = 0;
            while (b.dst[e] < p1) ++e;
            b.src[e] = p1 + ((b.src[e] - p1 + 7) % 40);
            expect_reject(dflt, b, {0, 0, 0, 3, 4}, false, "(pp edge", false);
        }
        {   // host rows that differ
            Batch b = cp;
            b.x[(size_t)(b.prot_ptr[2] + 5) * 3 + 1] += 0.01f;
            expect_reject(dflt, b, {0, 0, 0, 3, 4}, true, "coordinates / features differ", false);
            // ... which a device-resident batch cannot show on the host: accepted here, compared on the device
            const Tables t = run(inputs_of(dflt, b, false, true, {0, 0, 0, 3, 4}));
            CHECK(t.rc == PF_OK, "device rows: %s", t.msg.c_str());
        }
        // graph 3 has as many atoms as graph 0 but is another pocket: edge count, in-degrees or sources expose it
        {
            const BindInputs in = inputs_of(dflt, cp, false, true, {0, 0, 0, 0, 4});
            const Tables t = run(in);
            CHECK(t.rc == PF_ERR_ARG && t.msg.find("not a copy of graph 0") != std::string::npos, "another pocket of equal size: %d \"%s\"", t.rc, t.msg.c_str());
        }
    }
    if (g_fail) { printf("bind_check: %d checks FAILED\n", g_fail); return 1; }
    printf("bind_check: all checks passed\n");
    return 0;
}
