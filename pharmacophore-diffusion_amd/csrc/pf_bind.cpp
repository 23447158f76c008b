// pf_bind.cpp -- the bind planner (pf_bind.h): host only.
#include "pf_bind.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace pfbind {

#define BIND_FAIL(...)                                          \
    do {                                                        \
        char _b[512];                                           \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                  \
        err.msg = _b;                                           \
        return PF_ERR_ARG;                                      \
    } while (0)

// The pass over the pp edges for the common case -- destination-sorted, every edge inside its graph -- with 8 edges per
// instruction (a training loop binds a new batch every step: 0.65 M edges at 256 pockets, and the bind is on the step's
// host-side critical path).  Returns false when anything is unusual (unsorted, out of range, an edge across graphs): the
// scalar pass then runs and reports.  On success start[d] (d = 0 .. Np) = index of the first edge whose destination
// is >= d, i.e. the in-edge ranges of a destination-sorted list.
#if defined(__x86_64__)
__attribute__((target("avx2"))) static bool pp_edges_fast_avx2(const int* src, const int* dst, int64_t n, const int* prot_ptr, int B, int Np,
                                                                int* start) {
    if (n <= 0 || dst[0] < 0 || dst[n - 1] >= Np) return false;
    // sortedness + boundaries in one sweep: a boundary after edge e (dst[e] < dst[e + 1]) starts the ranges of nodes dst[e] + 1 .. dst[e + 1]
    for (int d = 0; d <= dst[0]; ++d) start[d] = 0;
    int64_t e = 0;
    for (; e + 8 < n; e += 8) {
        const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(dst + e));
        const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(dst + e + 1));
        if (_mm256_movemask_epi8(_mm256_cmpgt_epi32(a, b))) return false;                       // descending somewhere
        unsigned m = (unsigned)_mm256_movemask_ps(_mm256_castsi256_ps(_mm256_cmpgt_epi32(b, a)));
        while (m) {
            const int k = __builtin_ctz(m);
            m &= m - 1;
            const int lo = dst[e + k], hi = dst[e + k + 1];
            for (int d = lo + 1; d <= hi; ++d) start[d] = (int)(e + k + 1);
        }
    }
    for (; e + 1 < n; ++e) {
        if (dst[e] > dst[e + 1]) return false;
        for (int d = dst[e] + 1; d <= dst[e + 1]; ++d) start[d] = (int)(e + 1);
    }
    for (int d = dst[n - 1] + 1; d <= Np; ++d) start[d] = (int)n;
    // every source inside the atom range of its destination's graph (the destinations of graph g are the edges start[p0] .. start[p1])
    for (int g = 0; g < B; ++g) {
        const int lo = prot_ptr[g], hi = prot_ptr[g + 1];
        const int64_t a = start[lo], b = start[hi];
        const __m256i vlo = _mm256_set1_epi32(lo), vhi = _mm256_set1_epi32(hi);
        __m256i bad = _mm256_setzero_si256();
        int64_t i = a;
        for (; i + 8 <= b; i += 8) {
            const __m256i x = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i));
            bad = _mm256_or_si256(bad, _mm256_or_si256(_mm256_cmpgt_epi32(vlo, x), _mm256_cmpgt_epi32(x, _mm256_sub_epi32(vhi, _mm256_set1_epi32(1)))));
        }
        if (_mm256_movemask_epi8(bad)) return false;
        for (; i < b; ++i) if (src[i] < lo || src[i] >= hi) return false;
    }
    return true;
}
#else
static bool pp_edges_fast_avx2(const int*, const int*, int64_t, const int*, int, int, int*) { return false; }
#endif

int active_atoms(const pf_config& c, int np, int nf) {
    return c.pf_k > 0 ? std::min(np, nf * std::min(c.pf_k, np)) : (nf > 0 ? np : 0);
}

static size_t rnd256(size_t b) { return (b + 255) & ~size_t(255); }

int plan_batch(const BindInputs& in, BindPlan& out, BindError& err) {
    err = BindError{};
    const pf_config& c = in.cfg;
    const int B = in.B;
    const int32_t *prot_ptr = in.prot_ptr, *pharm_ptr = in.pharm_ptr, *pp_src = in.pp_src, *pp_dst = in.pp_dst;
    const int64_t n_pp = in.n_pp;
    if (B < 1 || !prot_ptr || !pharm_ptr || (in.host_rows && (!in.host_prot_x || !in.host_prot_h)) || n_pp < 0 || (n_pp && (!pp_src || !pp_dst)))
        BIND_FAIL("pf_set_pocket_batch: bad argument");
    if (prot_ptr[0] != 0 || pharm_ptr[0] != 0) BIND_FAIL("ptr arrays must start at 0");
    for (int g = 0; g < B; ++g) {
        if (prot_ptr[g + 1] < prot_ptr[g] || pharm_ptr[g + 1] < pharm_ptr[g]) BIND_FAIL("ptr arrays must be non-decreasing");
        if (pharm_ptr[g + 1] - pharm_ptr[g] > PF_MAXF)
            BIND_FAIL("graph %d has %d pharmacophore centers (limit %d)", g, pharm_ptr[g + 1] - pharm_ptr[g], PF_MAXF);
    }
    BindPlan p;
    const int Np = prot_ptr[B], Nf = pharm_ptr[B], N = Np + Nf;
    p.B = B; p.Np = Np; p.Nf = Nf; p.N = N; p.n_pp = n_pp;
    std::vector<int>& gid = p.gid;
    gid.resize(N);
    for (int g = 0; g < B; ++g) {
        p.max_np = std::max(p.max_np, prot_ptr[g + 1] - prot_ptr[g]);
        p.max_nf = std::max(p.max_nf, pharm_ptr[g + 1] - pharm_ptr[g]);
        for (int i = prot_ptr[g]; i < prot_ptr[g + 1]; ++i) gid[i] = g;
        for (int i = pharm_ptr[g]; i < pharm_ptr[g + 1]; ++i) gid[Np + i] = g;
    }
    // One pass over the pp edges checks them and counts the in-degrees (a training loop binds a new batch every step and
    // the bind is most of that step's host time): the graph of an edge is looked up only when the destination leaves
    // the atom range of the previous edge's graph -- edge lists come grouped by destination.
    std::vector<int>& deg = p.deg;
    deg.assign(Np + 1, 0);
    // radius_graph and pf_build_pp_edges emit the edges grouped by destination, ascending (the common case, 8 edges at a
    // time): fill_tables' stable sort is then the identity and is skipped
    const bool deg_is_prefix = in.allow_avx2 && pp_edges_fast_avx2(pp_src, pp_dst, n_pp, prot_ptr, B, Np, deg.data());
    if (!deg_is_prefix) {
        std::fill(deg.begin(), deg.end(), 0);
        // (per-edge increments, no branch on a change of destination: counting per run of equal destinations costs a
        // mispredicted branch per atom and measured 0.3 ms slower at 256 pockets)
        int prev_dst = -1, lo = 0, hi = 0;
        bool sorted = true;
        for (int64_t e = 0; e < n_pp; ++e) {
            const int sn = pp_src[e], dn = pp_dst[e];
            if ((unsigned)sn >= (unsigned)Np || (unsigned)dn >= (unsigned)Np) BIND_FAIL("pp edge %lld out of range", (long long)e);
            if (dn < lo || dn >= hi) { const int g = gid[dn]; lo = prot_ptr[g]; hi = prot_ptr[g + 1]; }
            if (sn < lo || sn >= hi) BIND_FAIL("pp edge %lld crosses graphs", (long long)e);
            sorted &= dn >= prev_dst;
            prev_dst = dn;
            deg[dn + 1]++;
        }
        p.dst_sorted = sorted;
    }
    // message_norm == 0 with kNN pf edges: the reference derives the per-graph pf / fp edge counts by looking the
    // pharmacophore-CENTER index of every edge up in the PROTEIN batch vector (dynamics_gvp.py:220), i.e. the min(k, Np_g)
    // edges of center j are booked on the graph that owns protein atom j.  gvp.py:506 normalises with those counts, so
    // they are reproduced (a pure function of the ptr arrays); the reference raises an IndexError when j >= Np_tot.
    if (c.message_norm_mode == PF_NORM_GRAPH && c.pf_k > 0) {
        p.pfq.assign(B, 0);
        for (int g = 0; g < B; ++g) {
            const int kg = std::min(c.pf_k, prot_ptr[g + 1] - prot_ptr[g]);
            if (kg > 0 && pharm_ptr[g + 1] > pharm_ptr[g] && pharm_ptr[g + 1] - 1 >= Np)
                BIND_FAIL("message_norm 0 with kNN pf edges: center index %d >= %d protein atoms "
                          "(the reference indexes the protein batch vector with it, dynamics_gvp.py:220)", pharm_ptr[g + 1] - 1, Np);
            for (int j = pharm_ptr[g]; j < pharm_ptr[g + 1] && kg > 0; ++j) p.pfq[gid[j]] += kg;
        }
    }
    if (!in.rep.empty() && (int)in.rep.size() != B)
        BIND_FAIL("pf_set_pocket_groups named %d graphs, this batch has %d", (int)in.rep.size(), B);
    // ---- (what follows reads only the ptr arrays, the degrees and the knobs: the caller's point of no return lay here)
    if (!deg_is_prefix)
        for (int i = 0; i < Np; ++i) deg[i + 1] += deg[i];
    // capacity of dynamic regions: ff, pf, fp and "pa" = compact copy of the pp edges into the active atoms
    p.h_reg.assign((size_t)4 * B, 0);
    p.h_cap.assign((size_t)4 * B, 0);
    p.reg_act.assign(B, 0); p.cap_act.assign(B, 0); p.maxdeg.assign(B, 0); p.epp_g.assign(B, 0);
    for (int i = 0; i < Np; ++i) {
        p.maxdeg[gid[i]] = std::max(p.maxdeg[gid[i]], deg[i + 1] - deg[i]);
        p.epp_g[gid[i]] += deg[i + 1] - deg[i];
    }
    int64_t cursor = n_pp;
    for (int et = 0; et < 4; ++et)
        for (int g = 0; g < B; ++g) {
            const int np = prot_ptr[g + 1] - prot_ptr[g], nf = pharm_ptr[g + 1] - pharm_ptr[g];
            int cap;
            if (et == ET_FF) cap = c.ff_k > 0 ? nf * std::min(c.ff_k, std::max(nf - 1, 0)) : nf * std::max(nf - 1, 0);
            else if (et < 3) cap = c.pf_k > 0 ? nf * std::min(c.pf_k, np) : nf * np;
            else {
                const int nact = active_atoms(c, np, nf);
                cap = (int)std::min<int64_t>(p.epp_g[g], (int64_t)nact * p.maxdeg[g]);
                p.reg_act[g] = p.act_total; p.cap_act[g] = nact; p.act_total += nact;
            }
            cursor = (cursor + 31) & ~int64_t(31);     // tiles are aligned to multiples of 32 slots (seg_tail in the kernels)
            p.h_reg[(size_t)et * B + g] = (int)cursor;
            p.h_cap[(size_t)et * B + g] = cap;
            cursor += cap;
        }
    if (cursor > 0x7fffffffLL / 128) { err.batch_lost = true; BIND_FAIL("edge capacity too large"); }
    p.Ecap = cursor;
    const int64_t Ecap = std::max<int64_t>(cursor, 1);
    // tiles: dynamic etypes first (they feed the short pharm-side chain), then pp
    std::vector<EdgeTile>& et_tiles = p.et_tiles;
    et_tiles.reserve((size_t)n_pp / 32 + (size_t)(Ecap - n_pp) / 8 + 64);
    for (int et = 0; et < 3; ++et) {
        p.et_tile0[et] = (int)et_tiles.size();
        for (int g = 0; g < B; ++g) {
            const int cap = p.h_cap[(size_t)et * B + g], reg = p.h_reg[(size_t)et * B + g];
            for (int o = 0; o < cap; o += 32) et_tiles.push_back({reg + o, std::min(32, cap - o), et, et * B + g, o});
        }
        // The output of the last conv layer is consumed only on the pharm nodes (dynamics_gvp.py:91), so in
        // that layer only the etypes with a pharm destination (ff, pf: the first tiles) and only the pharm node
        // tiles are computed; the reference computes and discards the protein side.
        if (et == ET_PF) p.n_edge_tiles_last = (int)et_tiles.size();
    }
    p.et_tile0[3] = (int)et_tiles.size();
    for (int64_t o = 0; o < n_pp; o += 32) et_tiles.push_back({(int)o, (int)std::min<int64_t>(32, n_pp - o), ET_PP, -1, 0});
    p.et_tile0[4] = (int)et_tiles.size();
    p.n_tiles.reserve((size_t)N / 32 + 8);
    for (int o = 0; o < Nf; o += 32) {
        p.n_tiles.push_back({Np + o, std::min(32, Nf - o), 1, -1, 0, 0});
        p.h_tiles.push_back({Np + o, std::min(32, Nf - o), 1, -1, 0, 0});
    }
    for (int o = 0; o < Np; o += 32) p.n_tiles.push_back({o, std::min(32, Np - o), 0, -1, 0, 0});
    p.n_edge_tiles = (int)et_tiles.size();
    p.n_node_tiles = (int)p.n_tiles.size();
    p.n_head_tiles = (int)p.h_tiles.size();
    p.n_node_tiles_last = (int)p.h_tiles.size();          // pharm tiles come first in n_tiles
    // pruned layer: ff, pf, fp tiles + pa tiles; pharm node tiles + tiles over the active-atom lists
    for (int et = 0; et < 4; ++et) {
        p.et_tile0_act[et] = (int)p.et_act.size();
        for (int g = 0; g < B; ++g) {
            const int cap = p.h_cap[(size_t)et * B + g], reg = p.h_reg[(size_t)et * B + g];
            for (int o = 0; o < cap; o += 32) p.et_act.push_back({reg + o, std::min(32, cap - o), et == 3 ? (int)ET_PP : et, et * B + g, o});
        }
    }
    p.et_tile0_act[4] = (int)p.et_act.size();
    p.n_act = p.h_tiles;
    for (int g = 0; g < B; ++g)
        for (int o = 0; o < p.cap_act[g]; o += 32) p.n_act.push_back({p.reg_act[g] + o, std::min(32, p.cap_act[g] - o), 0, 4 * B + g, o, 1});
    p.n_edge_tiles_act = (int)p.et_act.size();
    p.n_node_tiles_act = (int)p.n_act.size();
    // ---- layout: [table section: host-built, uploaded with one copy, a buffer of its own] and the workspace [zero section][scratch]
    const size_t n_eta = p.et_act.size() + 16, n_nta = p.n_act.size() + 16, n_et = et_tiles.size() + 16, n_nt = p.n_tiles.size() + 16,
                 n_ht = p.h_tiles.size() + 16;
    size_t off = 0;
    auto place = [&](size_t b) { const size_t o = off; off += rnd256(b); return o; };
    TableOff& t = p.t;
    t.pptr = place((B + 1) * 4); t.fptr = place((B + 1) * 4); t.gid = place((size_t)N * 4); t.reg = place((size_t)4 * B * 4);
    t.regact = place((size_t)B * 4); t.eta = place(n_eta * sizeof(EdgeTile)); t.nta = place(n_nta * sizeof(NodeTile));
    t.esrc = place(Ecap * 4); t.edst = place(Ecap * 4); t.ins = place((size_t)4 * N * 4); t.inc = place((size_t)4 * N * 4);
    t.ppc = place((size_t)B * 4); t.et = place(n_et * sizeof(EdgeTile)); t.nt = place(n_nt * sizeof(NodeTile));
    t.ht = place(n_ht * sizeof(NodeTile)); t.pfq = place((size_t)B * 4);
    t.regs = place((size_t)4 * B * 4); t.pas = place((size_t)B * 4); t.repb = place((size_t)B * 4);
    p.index_bytes = off;
    t.px0 = place((size_t)Np * 3 * 4 + 16); t.ph0 = place((size_t)Np * c.rec_nf * 4 + 16);
    p.table_bytes = in.host_rows ? off : p.index_bytes;      // what the single upload covers
    p.table_total = off;
    off = 0;                                                 // the workspace proper starts with the zero section
    // zero section (cleared with one launch per bind)
    ZeroOff& z = p.z;
    z.dyn = place((size_t)5 * B * 4); z.act = place((size_t)(p.act_total + 1) * 4); z.flag = place(256); z.gnorm = place((size_t)2 * B * 4);
    z.need = place((size_t)std::max(Np, 1) * 4);
    z.lpart = place(64 + (size_t)((Nf + 63) / 64) * 8 * sizeof(float));       // k_loss_eval's ticket (re-armed by its last block) + partial sums
    z.pastamp = place((size_t)std::max(Np, 1) * 4); z.pasame = place((size_t)B * 4);      // speculative "pa" messages: per-atom step stamps, per-graph verdicts
    z.pacnt = place((size_t)(B + 1) * 4);                                                 // ... the kind-3 counts they are mapped on (+ PFDYN_PA_SPEC_SPLIT's k)
    z.pagst = place(in.pa_check ? (size_t)(Ecap / 16 + 1) * 4 : 16);                      // PFDYN_PA_CHECK: per-group stamps
    p.zero_bytes = off;
    // scratch
    // (a second set of message rows for the last conv layer: the fused launch of small n_convs = 2 batches writes them while conv
    // layer 0's are still being read)
    p.msg2 = !in.wide && c.n_convs == 2 && (long)p.n_edge_tiles_act * 32 <= in.n16_rows_max;
    // node state and message rows at the handle's widths; the tables of the specialised path's hoists only where it runs
    const size_t S = (size_t)c.n_hidden_scalars, V3 = (size_t)3 * c.vector_size, SP = PF_S;
    auto spec_only = [&](size_t b) { return in.spec ? b : (size_t)16; };
    p.rec_slots = B <= 64 ? Ecap : 0;      // edge records: small batches only (the n16 fused launch)
    ScratchOff& s = p.s;
    s.xn = place((size_t)N * 16);
    s.fh = place((size_t)Nf * c.pharm_nf * 4 + 16); s.t = place((size_t)B * 4);
    s.h0 = place((size_t)N * S * 4); s.h1 = place((size_t)N * S * 4); s.v0 = place((size_t)N * V3 * 4); s.v1 = place((size_t)N * V3 * 4);
    s.ms = place((size_t)(Ecap + 1) * S * 4); s.mv = place((size_t)(Ecap + 1) * V3 * 4);
    s.ms2 = place(p.msg2 ? (size_t)(Ecap + 1) * PF_S * 4 : 16); s.mv2 = place(p.msg2 ? (size_t)(Ecap + 1) * 48 * 4 : 16);
    s.eh = place((size_t)Nf * c.pharm_nf * 4 + 16); s.ex = place((size_t)Nf * 3 * 4 + 16); s.c0 = place((size_t)B * 3 * 4); s.c1 = place((size_t)B * 3 * 4);
    s.pre = place(spec_only((size_t)std::max(Np, 1) * SP * 4)); s.eorig = place(Ecap * 4); s.ptype = place((size_t)std::max(Np, 1) * 4);
    s.rec = place((size_t)(in.edge_rec ? 3 * p.rec_slots : 0) * 16 + 16);
    s.zs = place(spec_only((size_t)std::max<int64_t>(n_pp, 1) * SP * 4)); s.ptpg = place(spec_only((size_t)B * L0_NTAB * c.rec_nf * SP * 4));
    s.xchg = place((size_t)2 * std::max(Nf, 1) * PF_XCHG_STRIDE * sizeof(unsigned int));      // (+ the center hoist's copy)
    s.cenh = place(spec_only((size_t)std::max(Nf, 1) * SP * 4)); s.cenp = place(spec_only((size_t)2 * std::max(Nf, 1) * SP * 4));
    s.snap = place((size_t)2 * (std::max(Nf, 1) * c.pharm_nf + 4) * 4);
    p.ws_bytes = off;
    out = std::move(p);
    return PF_OK;
}

int fill_tables(const BindPlan& p, const BindInputs& in, void* dst, FillResult& res, BindError& err) {
    err = BindError{};
    res = FillResult{};
    const pf_config& c = in.cfg;
    const int B = p.B, Np = p.Np, N = p.N;
    const int64_t n_pp = p.n_pp, Ecap = std::max<int64_t>(p.Ecap, 1);
    const int32_t *prot_ptr = in.prot_ptr, *pharm_ptr = in.pharm_ptr, *pp_src = in.pp_src, *pp_dst = in.pp_dst;
    const std::vector<int>&deg = p.deg, &epp_g = p.epp_g;
    const TableOff& t = p.t;
    char* const st = static_cast<char*>(dst);
    // pp edges sorted by destination (stable counting sort): CSR-by-dst.  The big index arrays are built in the staging
    // buffer itself (5 MB of edges and 2 MB of in-edge ranges at 256 pockets: no intermediate copies)
    int* const esrc = reinterpret_cast<int*>(st + t.esrc);
    int* const edst = reinterpret_cast<int*>(st + t.edst);
    int* const in_start = reinterpret_cast<int*>(st + t.ins);      // [4 slots][N]: BuildParams::in_start
    int* const in_cnt = reinterpret_cast<int*>(st + t.inc);
    int* const pp_cnt = reinterpret_cast<int*>(st + t.ppc);
    memset(esrc + n_pp, 0, (size_t)(Ecap - n_pp) * 4);
    memset(edst + n_pp, 0, (size_t)(Ecap - n_pp) * 4);
    memset(in_start, 0, (size_t)4 * N * 4);
    memset(in_cnt, 0, (size_t)4 * N * 4);
    if (p.dst_sorted) {
        if (n_pp > 0) { memcpy(esrc, pp_src, (size_t)n_pp * 4); memcpy(edst, pp_dst, (size_t)n_pp * 4); }
    } else {
        std::vector<int> fill(deg.begin(), deg.end() - 1);
        for (int64_t e = 0; e < n_pp; ++e) {
            const int pos = fill[pp_dst[e]]++;
            esrc[pos] = pp_src[e];
            edst[pos] = pp_dst[e];
        }
    }
    for (int g = 0; g < B; ++g) pp_cnt[g] = epp_g[g];
    for (int i = 0; i < Np; ++i) { in_start[(size_t)N + i] = deg[i]; in_cnt[(size_t)N + i] = deg[i + 1] - deg[i]; }
    // ---- pocket sharing (pf_set_pocket_groups): verify the caller's claim and prepare the tables of the sharing mode
    int* const regs = reinterpret_cast<int*>(st + t.regs);
    int* const pa_static = reinterpret_cast<int*>(st + t.pas);
    int* const rep_base = reinterpret_cast<int*>(st + t.repb);
    memcpy(regs, p.h_reg.data(), (size_t)4 * B * 4);
    memset(pa_static, 0, (size_t)B * 4);
    memset(rep_base, 0, (size_t)B * 4);
    res.h_share_start.assign(B, 0); res.h_share_cnt.assign(B, 0);
    if (!in.rep.empty()) {
        const std::vector<int>& rep = in.rep;
        long dense = 0, percopy = 0;
        int nrep = 0;
        for (int g = 0; g < B; ++g) {
            const int r = rep[g];
            if (r < 0 || r >= B || rep[r] != r) BIND_FAIL("pf_set_pocket_groups: graph %d names %d, which is not a representative", g, r);
            const int np = prot_ptr[g + 1] - prot_ptr[g];
            if (np != prot_ptr[r + 1] - prot_ptr[r] || epp_g[g] != epp_g[r])
                BIND_FAIL("pf_set_pocket_groups: graph %d is not a copy of graph %d (%d vs %d atoms, %d vs %d pp edges)",
                          g, r, np, prot_ptr[r + 1] - prot_ptr[r], epp_g[g], epp_g[r]);
            if (r != g) {
                // same static graph: in-degrees and (destination-sorted) sources, pocket-local
                const int p0g = prot_ptr[g], p0r = prot_ptr[r];
                for (int i = 0; i < np; ++i)
                    if (deg[p0g + i + 1] - deg[p0g + i] != deg[p0r + i + 1] - deg[p0r + i])
                        BIND_FAIL("pf_set_pocket_groups: graph %d is not a copy of graph %d (pp in-degree of atom %d)", g, r, i);
                const int eg = deg[p0g], er = deg[p0r];
                for (int k = 0; k < epp_g[g]; ++k)
                    if (esrc[eg + k] - p0g != esrc[er + k] - p0r)
                        BIND_FAIL("pf_set_pocket_groups: graph %d is not a copy of graph %d (pp edge %d)", g, r, k);
                if (in.host_rows && (memcmp(in.host_prot_x + (size_t)p0g * 3, in.host_prot_x + (size_t)p0r * 3, (size_t)np * 12) ||
                                     memcmp(in.host_prot_h + (size_t)p0g * c.rec_nf, in.host_prot_h + (size_t)p0r * c.rec_nf, (size_t)np * c.rec_nf * 4)))
                    BIND_FAIL("pf_set_pocket_groups: graph %d is not a copy of graph %d (coordinates / features differ)", g, r);
            } else { dense += epp_g[g]; ++nrep; }
            // what the per-copy form computes for this graph: the pp in-edges of its active atoms -- at most nf k
            // of them, about 60 % of that once the centers' neighbour sets overlap -- at the pocket's mean in-degree
            const int nact = active_atoms(c, np, pharm_ptr[g + 1] - pharm_ptr[g]);
            percopy += np > 0 ? (long)(0.6 * nact * (double)epp_g[g] / np) : 0;
        }
        // worth it when the representatives' static edges are clearly fewer than the per-copy edges they replace (about
        // half of them at 30 copies of a 256-atom pocket); the compact work list must cover 4 B regions
        // (with the per-step need stamps only the union of the copies' active atoms is computed, so what a
        // representative costs beyond that is launching the idle groups of its static range)
        res.share = nrep < B && 4 * B <= 1024 && (dense * 4 <= percopy * 3 || nrep * 4 <= B);
        if (res.share) {
            for (int g = 0; g < B; ++g) {
                const int r = rep[g], p0g = prot_ptr[g], p0r = prot_ptr[r], np = prot_ptr[g + 1] - p0g;
                for (int i = 0; i < np; ++i) {         // slot 3: the representative's static in-edge range of the same atom
                    in_start[(size_t)3 * N + p0g + i] = deg[p0r + i];
                    in_cnt[(size_t)3 * N + p0g + i] = deg[p0r + i + 1] - deg[p0r + i];
                }
                rep_base[g] = p0r;
                if (r == g) { res.h_share_start[g] = deg[p0g]; res.h_share_cnt[g] = epp_g[g]; }
                regs[(size_t)3 * B + g] = res.h_share_start[g];
                pa_static[g] = res.h_share_cnt[g];
            }
            res.share_rows = dense;
            for (int et = 0; et < 3; ++et) for (int g = 0; g < B; ++g) res.share_rows += p.h_cap[(size_t)et * B + g];
        }
    }
    // ---- the small tables
    memcpy(st + t.pptr, prot_ptr, (size_t)(B + 1) * 4);
    memcpy(st + t.fptr, pharm_ptr, (size_t)(B + 1) * 4);
    if (N > 0) memcpy(st + t.gid, p.gid.data(), (size_t)N * 4);
    memcpy(st + t.reg, p.h_reg.data(), (size_t)4 * B * 4);
    memcpy(st + t.regact, p.reg_act.data(), (size_t)B * 4);
    if (!p.et_act.empty()) memcpy(st + t.eta, p.et_act.data(), p.et_act.size() * sizeof(EdgeTile));
    if (!p.n_act.empty()) memcpy(st + t.nta, p.n_act.data(), p.n_act.size() * sizeof(NodeTile));
    if (!p.et_tiles.empty()) memcpy(st + t.et, p.et_tiles.data(), p.et_tiles.size() * sizeof(EdgeTile));
    if (!p.n_tiles.empty()) memcpy(st + t.nt, p.n_tiles.data(), p.n_tiles.size() * sizeof(NodeTile));
    if (!p.h_tiles.empty()) memcpy(st + t.ht, p.h_tiles.data(), p.h_tiles.size() * sizeof(NodeTile));
    if (!p.pfq.empty()) memcpy(st + t.pfq, p.pfq.data(), (size_t)B * 4);
    if (in.host_rows) {
        if (Np > 0) {
            memcpy(st + t.px0, in.host_prot_x, (size_t)Np * 3 * 4);
            memcpy(st + t.ph0, in.host_prot_h, (size_t)Np * c.rec_nf * 4);
        }
        // the one-hot verdict (static hoist) on the host copy: nobody will wait for the device-side check
        res.host_onehot = Np > 0 ? 1 : 0;
        for (int i = 0; i < Np && res.host_onehot; ++i) {
            int ones = 0;
            for (int k = 0; k < c.rec_nf; ++k) {
                const float x = in.host_prot_h[(size_t)i * c.rec_nf + k];
                if (x == 1.0f) ++ones; else if (x != 0.0f) res.host_onehot = 0;
            }
            if (ones != 1) res.host_onehot = 0;
        }
    }
    return PF_OK;
}

}  // namespace pfbind
