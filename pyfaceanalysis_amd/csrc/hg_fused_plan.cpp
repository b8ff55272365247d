// The planner of the fused executor, host only: the normal form of a flow tree (folded affines, layer groups, composed
// Switchboards) and, from it, the plan the kernels run from (hg_fused_plan.hpp) — weight fragments permuted to fragment order,
// bias vectors, K-block tables with the Switchboards folded in, the stage-0 chunk / run tables, remainder-tile and packed-block
// decisions, the top-of-hierarchy launch and the sub-tree runs, and the stage names hg_flow_describe prints.  No HIP call: the
// executor (hg_fused.hip) uploads the finished plan and never writes to it.  Data layout: see hg_fused.hip.
#include <algorithm>
#include <cmath>
#include <map>
#include <sstream>
#include <tuple>

#include "hg_fused_plan.hpp"
#include "hg_fused_stages.hpp"

namespace hg {
namespace fused {

namespace {

// ---- host-side normal form (Aff, FNode, FStage: hg_fused_stages.hpp) ------------------------------
Aff aff_of(const TNode& n) { return Aff{(int)n.in_dim, (int)n.out_dim, n.a, n.W, n.b}; }

Aff fold(const Aff& f, const Aff& s) {  // s(f(x)) = (x - f.a)(f.W s.W) + (f.b - s.a) s.W + s.b
    Aff r;
    r.in = f.in;
    r.out = s.out;
    r.a = f.a;
    r.W.assign((size_t)f.in * s.out, 0.0);
    for (int i = 0; i < f.in; ++i)
        for (int k = 0; k < f.out; ++k) {
            double w = f.W[(size_t)i * f.out + k];
            if (w == 0.0) continue;
            for (int j = 0; j < s.out; ++j) r.W[(size_t)i * s.out + j] += w * s.W[(size_t)k * s.out + j];
        }
    r.b = s.b;
    for (int k = 0; k < f.out; ++k) {
        double d = f.b[k] - s.a[k];
        for (int j = 0; j < s.out; ++j) r.b[j] += d * s.W[(size_t)k * s.out + j];
    }
    return r;
}

typedef std::vector<const TNode*> LeafSeq;

bool flatten_leafs(const TNode& n, LeafSeq& s, std::string& why) {
    switch (n.kind) {
        case K_AFFINE:
        case K_EXPANSION:
        case K_HEAD:
        case K_CUTOFF:
        case K_IGSFA: s.push_back(&n); return true;
        case K_IDENTITY: return true;
        case K_FLOWNODE:
        case K_FLOW:
            for (auto& c : n.ch)
                if (!flatten_leafs(*c, s, why)) return false;
            return true;
        default: why = std::string("node kind ") + kind_name(n.kind) + " inside a layer is not covered by the fused plan"; return false;
    }
}

struct ChainT {
    int in_dim, out_dim;
    LeafSeq seq;
};

bool to_chains(const TNode& n, std::vector<ChainT>& out, std::string& why) {
    auto one = [&](const TNode& c) {
        ChainT ch{(int)c.in_dim, (int)c.out_dim, {}};
        if (!flatten_leafs(c, ch.seq, why)) return false;
        out.push_back(std::move(ch));
        return true;
    };
    if (n.kind == K_LAYER) {
        for (auto& c : n.ch)
            if (!one(*c)) return false;
        return true;
    }
    if (n.kind == K_CLONELAYER) {
        for (uint32_t i = 0; i < n.aux; ++i)
            if (!one(*n.ch[0])) return false;
        return true;
    }
    return one(n);
}

// An iGSFA node is ONE affine map of its expanded input when the expansion contains the identity over all
// columns (e P = x0 for a selection matrix P):
//     s = e Ws + cs,           cs = bs - as Ws                       (scale already folded into Ws, bs)
//     l = e (Ws Wl) + cl,      cl = (cs - al) Wl + bl                (reconstruction, when present)
//     q = e (P - Ws Wl) Wp + (-cl - ap) Wp + bp
// so y = [s, q] = e [Ws | (P - Ws Wl) Wp] + const, folded here in float64.  Nodes of up to 64 inputs then run
// as ordinary nodes (first affine = x - mean, second = the folded map) on the kernels tuned for them —
// including the fused first-two-layers kernel, which also makes the k_im2frag pass unnecessary; the MFMA
// count is about the same (one GEMM over 2 d_in instead of three smaller ones).  Wider nodes stay on k_igsfa
// (their identity first affine would need more than kMaxMT tiles) but use the same folded map there: one GEMM
// from the expanded input fragments to all output tiles instead of the G1 -> G2 -> G3 chain.
// HIGSFA_IG_NOFOLD=1 keeps every iGSFA node on the three-GEMM form (tests).
bool igsfa_affine(const FNode& fn, Aff& A2, bool nofold) {
    const int d = fn.in_dim, k = fn.ig_k, q = fn.ig_pca.out;
    if (nofold) return false;
    int E = 0, id_off = -1;
    for (const ExpFunc& f : fn.funcs) {
        if (f.kind == E_IDENTITY && f.used(d) == d && id_off < 0) id_off = E;
        E += f.out_dim(d);
    }
    if (id_off < 0 || fn.ig_sfa.in != E || fn.ig_sfa.out != k) return false;
    const Aff &S = fn.ig_sfa, &Lr = fn.ig_lr, &Pc = fn.ig_pca;
    std::vector<double> cs(k), Wsl((size_t)E * d, 0.0), cl(d, 0.0);
    for (int j = 0; j < k; ++j) {
        double v = S.b[j];
        for (int e = 0; e < E; ++e) v -= S.a[e] * S.W[(size_t)e * k + j];
        cs[j] = v;
    }
    if (fn.ig_has_lr) {
        for (int e = 0; e < E; ++e)
            for (int j = 0; j < k; ++j) {
                const double w = S.W[(size_t)e * k + j];
                if (w == 0.0) continue;
                for (int c = 0; c < d; ++c) Wsl[(size_t)e * d + c] += w * Lr.W[(size_t)j * d + c];
            }
        for (int c = 0; c < d; ++c) {
            double v = Lr.b[c];
            for (int j = 0; j < k; ++j) v += (cs[j] - Lr.a[j]) * Lr.W[(size_t)j * d + c];
            cl[c] = v;
        }
    }
    A2 = Aff();
    A2.in = E;
    A2.out = k + q;
    A2.a.assign(E, 0.0);
    A2.W.assign((size_t)E * (k + q), 0.0);
    A2.b.assign(k + q, 0.0);
    for (int e = 0; e < E; ++e) {
        for (int j = 0; j < k; ++j) A2.W[(size_t)e * (k + q) + j] = S.W[(size_t)e * k + j];
        for (int c = 0; c < d; ++c) {
            const double m = ((e == id_off + c) ? 1.0 : 0.0) - Wsl[(size_t)e * d + c];
            if (m == 0.0) continue;
            for (int j = 0; j < q; ++j) A2.W[(size_t)e * (k + q) + k + j] += m * Pc.W[(size_t)c * q + j];
        }
    }
    for (int j = 0; j < k; ++j) A2.b[j] = cs[j];
    for (int j = 0; j < q; ++j) {
        double v = Pc.b[j];
        for (int c = 0; c < d; ++c) v += (-cl[c] - Pc.a[c]) * Pc.W[(size_t)c * q + j];
        A2.b[k + j] = v;
    }
    return true;
}

void fold_igsfa(FNode& fn, bool nofold) {
    const int d = fn.in_dim;
    Aff A2;
    if (d > 16 * kMaxMT || !igsfa_affine(fn, A2, nofold)) return;
    Aff A1;
    A1.in = A1.out = d;
    A1.a = fn.ig_mean;
    A1.a.resize(d, 0.0);
    A1.W.assign((size_t)d * d, 0.0);
    for (int c = 0; c < d; ++c) A1.W[(size_t)c * d + c] = 1.0;
    A1.b.assign(d, 0.0);
    fn.A1 = std::move(A1);
    fn.A2 = std::move(A2);
    fn.is_ig = false;
    fn.was_ig = true;
}

bool canon(const ChainT& c, int in_off, FNode& fn, std::string& why, const FusedOptions& opt) {
    fn.in_off = in_off;
    fn.in_dim = c.in_dim;
    fn.out_dim = c.out_dim;
    for (const TNode* l : c.seq)
        if (l->kind == K_IGSFA) {
            if (c.seq.size() != 1) { why = "iGSFA node combined with other nodes in one chain"; return false; }
            if (l->sfa->out_dim != l->aux) { why = "iGSFA node whose sfa_node has more outputs than it preserves"; return false; }
            if (l->in_dim > 128 || l->out_dim > 16 * kMaxMT) { why = "iGSFA node with more than 128 inputs or 64 outputs"; return false; }
            fn.is_ig = true;
            fn.ig_k = (int)l->aux;
            fn.ig_mean = l->x_mean;
            fn.ig_sfa = aff_of(*l->sfa);
            for (int r = 0; r < fn.ig_sfa.in; ++r)
                for (int cc = 0; cc < fn.ig_sfa.out; ++cc) fn.ig_sfa.W[(size_t)r * fn.ig_sfa.out + cc] *= l->magn[cc];
            {   // ((e - a) W + b) * magn = (e - a)(W magn) + b magn
                for (int cc = 0; cc < fn.ig_sfa.out; ++cc) fn.ig_sfa.b[cc] *= l->magn[cc];
            }
            fn.ig_has_lr = (bool)l->lr;
            if (l->lr) fn.ig_lr = aff_of(*l->lr);
            fn.ig_pca = aff_of(*l->pca);
            if (l->exp_node) {
                for (const ExpFunc& f : l->exp_node->funcs)
                    if (f.kind > E_SIGNED_POW) { why = "expansion with cross-column products (QT / pair products)"; return false; }
                fn.funcs = l->exp_node->funcs;
            } else {
                fn.funcs = {ExpFunc{E_IDENTITY, 0, 0, 1.0}};
            }
            fn.has_exp = true;
            fold_igsfa(fn, opt.ig_nofold);
            return true;
        }
    int phase = 0;  // 0: before A1, 1: in A1, 2: after E, 3: in A2
    auto head = [](Aff& a, int keep) {        // HeadNode after an affine: keep its first `keep` outputs
        Aff r;
        r.in = a.in;
        r.out = keep;
        r.a = a.a;
        r.W.resize((size_t)a.in * keep);
        for (int i = 0; i < a.in; ++i)
            for (int o = 0; o < keep; ++o) r.W[(size_t)i * keep + o] = a.W[(size_t)i * a.out + o];
        r.b.assign(a.b.begin(), a.b.begin() + keep);
        a = std::move(r);
    };
    for (const TNode* l : c.seq) {
        if (l->kind == K_AFFINE) {
            if (phase == 0) { fn.A1 = aff_of(*l); phase = 1; }
            else if (phase == 1) fn.A1 = fold(fn.A1, aff_of(*l));
            else if (phase == 2) { fn.A2 = aff_of(*l); phase = 3; }
            else fn.A2 = fold(fn.A2, aff_of(*l));
        } else if (l->kind == K_HEAD) {
            if (phase == 1) head(fn.A1, (int)l->out_dim);
            else if (phase == 3) head(fn.A2, (int)l->out_dim);
            else { why = "HeadNode that does not follow an affine node"; return false; }
        } else if (l->kind == K_CUTOFF) {
            if (phase != 2 || fn.has_clip) { why = "CutoffNode anywhere but between the expansion and the second affine"; return false; }
            fn.has_clip = true;
            fn.clip_lo = l->lo;
            fn.clip_hi = l->hi;
        } else {  // expansion
            if (phase != 1) { why = "node chain is not [affine][expansion][affine]"; return false; }
            for (const ExpFunc& f : l->funcs)
                if (f.kind > E_SIGNED_POW) fn.has_prod = true;
            fn.funcs = l->funcs;
            fn.has_exp = true;
            phase = 2;
        }
    }
    if (phase == 0) { why = "layer node without an affine part"; return false; }
    if (phase == 2) { why = "node chain ends in an expansion"; return false; }
    if (fn.A1.out > 16 * kMaxMT || (fn.has_exp && fn.A2.out > 16 * kMaxMT)) {
        why = "affine with more than 64 outputs";
        return false;
    }
    return true;
}

}  // namespace

bool build_stages(const TNode& root, std::vector<FStage>& stages, std::string& why, const FusedOptions& opt) {
    std::vector<int32_t> pending;  // composition of switchboards since the last layer group
    bool have_pending = false;
    std::vector<ChainT> group;
    int frame_w = root.in_dim;

    auto close_group = [&]() -> bool {
        if (group.empty()) return true;
        FStage st;
        int in_w = 0;
        for (auto& c : group) in_w += c.in_dim;
        if (have_pending) {
            if ((int)pending.size() != in_w) { why = "internal: connection count"; return false; }
            st.conn = pending;
        } else {
            if (in_w != frame_w) { why = "internal: frame width"; return false; }
            st.conn.resize(in_w);
            for (int i = 0; i < in_w; ++i) st.conn[i] = i;
        }
        int off = 0;
        for (auto& c : group) {
            FNode fn;
            if (!canon(c, off, fn, why, opt)) return false;
            off += c.in_dim;
            st.out_w += fn.out_dim;
            st.nodes.push_back(std::move(fn));
        }
        frame_w = st.out_w;
        stages.push_back(std::move(st));
        group.clear();
        pending.clear();
        have_pending = false;
        return true;
    };

    for (auto& cp : root.ch) {
        const TNode& c = *cp;
        if (c.kind == K_SWITCHBOARD) {
            if (!close_group()) return false;
            if (have_pending) {
                std::vector<int32_t> comp(c.conn.size());
                for (size_t i = 0; i < c.conn.size(); ++i) comp[i] = pending[c.conn[i]];
                pending.swap(comp);
            } else {
                pending = c.conn;
                have_pending = true;
            }
            continue;
        }
        if (c.kind == K_IDENTITY) continue;      // mdp IdentityNode between layers: nothing to execute
        std::vector<ChainT> chains;
        if (!to_chains(c, chains, why)) return false;
        bool merged = false;
        if (!group.empty() && group.size() == chains.size()) {
            merged = true;
            for (size_t k = 0; k < chains.size(); ++k)
                if (group[k].out_dim != chains[k].in_dim) { merged = false; break; }
            // merging [A][E][A] + another [A ...] is fine (folds); anything after A2 with an expansion is not
            if (merged)
                for (size_t k = 0; k < chains.size() && merged; ++k) {
                    int n_exp = 0, n_ig = 0;
                    for (auto* l : group[k].seq) { n_exp += l->kind == K_EXPANSION; n_ig += l->kind == K_IGSFA; }
                    for (auto* l : chains[k].seq) { n_exp += l->kind == K_EXPANSION; n_ig += l->kind == K_IGSFA; }
                    if (n_exp > 1 || n_ig > 0) merged = false;
                }
            if (merged)
                for (size_t k = 0; k < chains.size(); ++k) {
                    group[k].out_dim = chains[k].out_dim;
                    for (auto* l : chains[k].seq) group[k].seq.push_back(l);
                }
        }
        if (!merged) {
            if (!close_group()) return false;
            group = std::move(chains);
        }
    }
    if (!close_group()) return false;
    if (have_pending) { why = "flow ends in a switchboard"; return false; }
    if (stages.empty()) { why = "no layer in the flow"; return false; }
    return true;
}

namespace {
// One parent's share of a link, in float64: per child c (of `kids`) the folded matrix A2_c A1_p[rows of c, :] ([A2_c.in x P], W[c];
// the other entries of W stay empty) and the ONE bias vector b1_p + sum_c (b2_c - a_p[rows c]) A1_p[rows c, :] - sum_c a2_c W[c].
// owner / col0: column of the child frame -> child node / first column of a child.  Changes nothing: hoist_first_affines stores
// the result in the normal form, the link 0 -> 1 keeps it beside the two stages (Planner::plan_fold01).
struct LinkFold {
    std::vector<double> bias;
    std::vector<std::vector<double>> W;
};
LinkFold fold_link(const FStage& ch, const FStage& pa, int pj, const std::vector<int>& owner, const std::vector<int>& col0, const std::vector<int>& kids) {
    const FNode& pn = pa.nodes[pj];
    const int P = pn.A1.out;
    LinkFold lf;
    lf.bias = pn.A1.b;
    lf.W.resize(ch.nodes.size());
    for (int ci : kids) lf.W[ci].assign((size_t)ch.nodes[ci].A2.in * P, 0.0);
    for (int c = 0; c < pn.in_dim; ++c) {
        const int pc = pa.conn[pn.in_off + c], ci = owner[pc], k = pc - col0[ci];
        const Aff& A2 = ch.nodes[ci].A2;
        const double* w1 = &pn.A1.W[(size_t)c * P];
        const double d = A2.b[k] - pn.A1.a[c];
        for (int o = 0; o < P; ++o) lf.bias[o] += d * w1[o];
        std::vector<double>& W = lf.W[ci];
        for (int e = 0; e < A2.in; ++e) {
            const double w2 = A2.W[(size_t)e * A2.out + k];
            if (w2 == 0.0) continue;
            for (int o = 0; o < P; ++o) W[(size_t)e * P + o] += w2 * w1[o];
        }
    }
    for (int ci : kids) {
        const Aff& A2 = ch.nodes[ci].A2;
        for (int e = 0; e < A2.in; ++e) {
            const double a = A2.a[e];
            if (a == 0.0) continue;
            for (int o = 0; o < P; ++o) lf.bias[o] -= a * lf.W[ci][(size_t)e * P + o];
        }
    }
    return lf;
}

}  // namespace

// Hoisted links.  Between a child's second affine (y_c = e_c A2_c + const) and its parent's first affine (z_p = (x_p - a_p) A1_p) there
// is only a Switchboard, so where every child column is read exactly once, and all of one child's by one parent,
//     z_p = sum_c e_c (A2_c A1_p[rows of c, :]) + const_p:
// the child multiplies its expanded input by the folded matrix, stores z's partial tiles instead of its own output, and the parent
// adds its children's tiles and ONE bias vector — no first GEMM.  Taken where that makes the child's output no wider (P of the
// parent <= S of each child) and both stages are ordinary layers on plain 16-row tiles; the links into stage 1 and below stay
// (the front kernels read those stages' own layout).  Products stay fp32 MFMAs; the fold itself is float64, like fold() above.
std::vector<int> hoist_first_affines(std::vector<FStage>& fs, const FusedOptions& opt) {
    (void)opt;
    std::vector<int> parents;
    auto ordinary = [](const FStage& st) {
        for (auto& n : st.nodes)
            if (n.is_ig || n.has_prod || n.has_clip || !n.has_exp) return false;
        return true;
    };
    auto rem_tile = [](int d) {      // the last 16-row tile of d outputs holds 1..4 rows: a 4x4 remainder tile (or a packed block) could apply
        const int r = d - 16 * ((d + 15) / 16 - 1);
        return r >= 1 && r <= 4;
    };
    for (size_t l = 1; l + 1 < fs.size(); ++l) {
        FStage& ch = fs[l];
        FStage& pa = fs[l + 1];
        if (!ordinary(ch) || !ordinary(pa)) continue;
        const int nc = (int)ch.nodes.size(), np = (int)pa.nodes.size();
        std::vector<int> owner, col0(nc, 0);      // column of the child frame -> child node
        for (int ci = 0; ci < nc; ++ci) {
            col0[ci] = (int)owner.size();
            owner.insert(owner.end(), ch.nodes[ci].out_dim, ci);
        }
        std::vector<int> reads(owner.size(), 0), parent_of(nc, -1);
        std::vector<std::vector<int>> kids(np);
        bool ok = true;
        int p_max = 0;
        for (int pj = 0; pj < np && ok; ++pj) {
            const FNode& pn = pa.nodes[pj];
            p_max = std::max(p_max, pn.A1.out);
            if (pn.A1.in != pn.in_dim || !pn.sum_bias.empty()) ok = false;
            for (int c = 0; c < pn.in_dim && ok; ++c) {
                const int pc = pa.conn[pn.in_off + c];
                if (pc < 0 || pc >= (int)owner.size() || ++reads[pc] > 1) { ok = false; break; }
                const int ci = owner[pc];
                if (parent_of[ci] < 0) {
                    parent_of[ci] = pj;
                    kids[pj].push_back(ci);
                } else if (parent_of[ci] != pj) {
                    ok = false;
                }
            }
            if (kids[pj].empty() || kids[pj].size() > 8) ok = false;
        }
        for (int r : reads) ok = ok && r == 1;      // every child column is read by exactly one parent, exactly once
        for (int ci = 0; ci < nc && ok; ++ci) {
            if (parent_of[ci] < 0) { ok = false; break; }
            const FNode& cn = ch.nodes[ci];
            if (cn.A2.out != cn.out_dim || pa.nodes[parent_of[ci]].A1.out > cn.A2.out) ok = false;
        }
        if (!ok || rem_tile(p_max)) continue;

        for (int pj = 0; pj < np; ++pj) {
            FNode& pn = pa.nodes[pj];
            const int P = pn.A1.out;
            LinkFold lf = fold_link(ch, pa, pj, owner, col0, kids[pj]);
            pn.sum_bias = std::move(lf.bias);
            pn.kids = kids[pj];
            std::vector<std::vector<double>>& Wf = lf.W;
            for (int ci : kids[pj]) {
                FNode& cn = ch.nodes[ci];
                Aff f;
                f.in = cn.A2.in;
                f.out = P;
                f.a.assign(f.in, 0.0);
                f.W = std::move(Wf[ci]);
                f.b.assign(P, 0.0);
                cn.A2 = std::move(f);
                cn.out_dim = P;
            }
            pn.A1.a.clear();
            pn.A1.W.clear();
            pn.A1.b.clear();
        }
        ch.out_w = 0;
        for (auto& cn : ch.nodes) ch.out_w += cn.out_dim;
        pa.sum_in = true;
        parents.push_back((int)l + 1);
    }
    return parents;
}

namespace {

inline int q_of_row(int i) { return 4 * (i & 3) + (i >> 2); }  // tile row -> tile-local feature (involution)

constexpr int kStage0ChunkCols = 128;   // columns of one sub-image staged per chunk (T = 4 tiles -> ~66 KiB LDS)
// Builds a FusedPlan in place: the constructor plans stage by stage, the member functions are its steps.  It adds no state of
// its own, so build_fused_plan hands out the FusedPlan part alone.
struct Planner : FusedPlan {
    Planner(const TNode& root, std::vector<FStage>&& fs, const FusedOptions& options) {
        opt = options;
        out_dim = root.out_dim;
        std::vector<int32_t> prev_blk, prev_q;  // per column of the previous stage's output frame
        int prev_nb = 0;
        bool prev_packed = false;                // previous stage stores packed remainder tiles (its consumer decodes r0)
        for (size_t si = 0; si < fs.size(); ++si) {
            FStage& st = fs[si];
            if (st.nodes[0].is_ig) {
                if (stages.empty()) add_gather0(st, prev_blk, prev_q, prev_nb);
                build_ig_stage(st, prev_blk, prev_q, prev_nb);
                prev_packed = false;
                continue;
            }
            {
                bool table_driven = st.nodes[0].has_clip;
                for (auto& nd : st.nodes) table_driven = table_driven || nd.has_prod;
                if (table_driven) {
                    if (stages.empty()) add_gather0(st, prev_blk, prev_q, prev_nb);
                    build_prod_stage(st, prev_blk, prev_q, prev_nb, (int)si);
                    prev_packed = false;
                    continue;
                }
            }
            if (si > 0 && stages.empty()) fail(HG_ERR_FORMAT, "internal: stage order");
            stages.emplace_back();
            HostStage& hs = stages.back();
            hs.from_x = si == 0;
            const int n = (int)st.nodes.size();
            hs.n_nodes = n;
            hs.has_exp = st.nodes[0].has_exp;
            hs.funcs = st.nodes[0].funcs;
            hs.nf = (int)hs.funcs.size();
            int p_max = 0;
            for (auto& nd : st.nodes) {
                hs.mt1 = std::max(hs.mt1, (nd.A1.out + 15) / 16);
                if (nd.has_exp) hs.mt2 = std::max(hs.mt2, (nd.A2.out + 15) / 16);
                p_max = std::max(p_max, nd.A1.out);
                if (nd.has_exp) hs.s_max = std::max(hs.s_max, nd.A2.out);
            }
            hs.p_max = p_max;
            if (!hs.has_exp) hs.mt2 = 1;
            hs.mto = hs.has_exp ? hs.mt2 : hs.mt1;
            hs.nb_in = prev_nb;
            for (int mt1 = 0; mt1 < hs.mt1; ++mt1)
                for (int fi = 0; fi < hs.nf; ++fi) {
                    int valid = std::max(0, std::min(16, hs.funcs[fi].used(p_max) - 16 * mt1));
                    hs.nk2[mt1][fi] = (uint8_t)((valid + 3) / 4);
                }

            // ---- per node: K-blocks of GEMM 1 and, for every (kblock, q), the consumer input positions
            struct NodeK {
                std::vector<int> src, nk;
                std::vector<std::vector<int>> kpos;  // [kb*16 + q] -> positions c
            };
            std::vector<NodeK> nks(n);
            if (si == 0) plan_stage0_inputs(st, hs);
            for (int ni = 0; ni < n; ++ni) {
                FNode& nd = st.nodes[ni];
                NodeK& K = nks[ni];
                if (st.sum_in) {      // child-major: entry i is tile i % mt1 of child i / mt1 (the layer below stores whole blocks, mto = mt1)
                    const HostStage& below = stages[stages.size() - 2];
                    if (below.kind != 0 || below.pack_out || below.mto != hs.mt1) fail(HG_ERR_FORMAT, "internal: hoisted link over a layer of another layout");
                    for (int ci : nd.kids)
                        for (int mt = 0; mt < hs.mt1; ++mt) {
                            K.src.push_back(ci * below.mto + mt);
                            K.nk.push_back(1);      // (a flag here: the block is added, not multiplied)
                            for (int qq = 0; qq < 16; ++qq) K.kpos.emplace_back();
                        }
                } else if (si == 0) {
                    const int nkb = (nd.in_dim + 15) / 16;
                    for (int kb = 0; kb < nkb; ++kb) {
                        // K slot (k-step r, lane group g) <- input position s0_pos(r, g) of this block
                        int valid = std::min(16, nd.in_dim - kb * 16), nk = 0;
                        K.src.push_back(0);
                        for (int q = 0; q < 16; ++q) {
                            K.kpos.emplace_back();
                            const int pos = s0_pos(q >> 2, q & 3);
                            if (pos < valid) {
                                K.kpos.back().push_back(kb * 16 + pos);
                                nk = std::max(nk, (q >> 2) + 1);
                            }
                        }
                        K.nk.push_back(nk);
                    }
                } else {
                    std::map<int, int> blk_index;
                    for (int c = 0; c < nd.in_dim; ++c) {
                        int pc = st.conn[nd.in_off + c];
                        int blk = prev_blk[pc], q = prev_q[pc];
                        auto it = blk_index.find(blk);
                        int kb;
                        if (it == blk_index.end()) {
                            kb = (int)K.src.size();
                            blk_index[blk] = kb;
                            K.src.push_back(blk);
                            K.nk.push_back(0);
                            for (int qq = 0; qq < 16; ++qq) K.kpos.emplace_back();
                        } else {
                            kb = it->second;
                        }
                        K.kpos[kb * 16 + q].push_back(c);
                        K.nk[kb] = std::max(K.nk[kb], q / 4 + 1);
                    }
                }
                hs.kb1 = std::max(hs.kb1, (int)K.src.size());
            }
            hs.sum_in = st.sum_in;
            hs.n_kids = st.sum_in ? hs.kb1 / hs.mt1 : 0;
            const int a1_blocks = st.sum_in ? 0 : hs.kb1 * hs.mt1;      // a hoisted first affine has no fragments
            hs.node_blocks = a1_blocks + (hs.has_exp ? hs.mt1 * hs.nf * hs.mt2 : 0);
            hs.bias_floats = (hs.mt1 + (hs.has_exp ? hs.mt2 : 0)) * 16;
            if (si > 0 && (size_t)hs.node_blocks * 1024 + (size_t)hs.bias_floats * 4 + (size_t)hs.kb1 * 8 > 150 * 1024)
                fail(HG_ERR_FORMAT, "fused: one node needs %d KiB of weight fragments, more than a workgroup's LDS", hs.node_blocks);
            hs.afrag.assign((size_t)n * hs.node_blocks * 256, 0.f);
            hs.bias.assign((size_t)n * hs.bias_floats, 0.f);
            if (si > 0) hs.kb1tab.assign((size_t)n * hs.kb1 * 2, 0);

            std::vector<int32_t> cur_blk, cur_q, node_out;
            for (int ni = 0; ni < n; ++ni) {
                FNode& nd = st.nodes[ni];
                NodeK& K = nks[ni];
                const int p = nd.A1.out;
                float* wnode = hs.afrag.data() + (size_t)ni * hs.node_blocks * 256;
                float* bnode = hs.bias.data() + (size_t)ni * hs.bias_floats;
                // bias 1: (x - a) W + b = x W + (b - a W); stage 0 subtracts fl32(a) in the loader and
                // keeps only the fp64 remainder here
                std::vector<double> bias1 = st.sum_in ? nd.sum_bias : nd.A1.b;
                for (int c = 0; c < nd.in_dim && !st.sum_in; ++c) {
                    double av = si == 0 ? nd.A1.a[c] - (double)(float)nd.A1.a[c] : nd.A1.a[c];
                    if (av == 0.0) continue;
                    for (int o = 0; o < p; ++o) bias1[o] -= av * nd.A1.W[(size_t)c * p + o];
                }
                for (size_t kb = 0; kb < K.src.size(); ++kb) {
                    int r0 = 0;      // leading k-steps of a packed block that belong to other nodes' rows: skipped (k_stage only)
                    if (si > 0 && prev_packed) {
                        r0 = 4;
                        for (int q = 0; q < 16; ++q)
                            if (!K.kpos[kb * 16 + q].empty()) r0 = std::min(r0, q / 4);
                        if (r0 >= K.nk[kb]) r0 = 0;
                    }
                    if (si > 0) {
                        hs.kb1tab[((size_t)ni * hs.kb1 + kb) * 2] = K.src[kb];
                        hs.kb1tab[((size_t)ni * hs.kb1 + kb) * 2 + 1] = K.nk[kb] | (r0 << 8);
                    }
                    if (st.sum_in) continue;
                    hs.mfma_per_tile += (int64_t)(K.nk[kb] - r0) * hs.mt1;
                    hs.ks1_tile += K.nk[kb] - r0;
                    for (int mt = 0; mt < hs.mt1; ++mt) {
                        float* blk = wnode + ((size_t)kb * hs.mt1 + mt) * 256;
                        for (int lane = 0; lane < 64; ++lane) {
                            int i = lane & 15, gg = lane >> 4;
                            int fo = 16 * mt + q_of_row(i);
                            if (fo >= p) continue;
                            for (int r = 0; r < 4; ++r) {
                                double w = 0;
                                for (int c : K.kpos[kb * 16 + 4 * r + gg]) w += nd.A1.W[(size_t)c * p + fo];
                                blk[lane * 4 + r] = (float)w;
                            }
                        }
                    }
                }
                if (si > 0)  // padded K-blocks: any valid source block, zero k-steps
                    for (int kb = (int)K.src.size(); kb < hs.kb1; ++kb) hs.kb1tab[((size_t)ni * hs.kb1 + kb) * 2] = K.src[0];
                if (si == 0 && (int)K.src.size() == hs.kb1) hs.nk_last = std::max(ni == 0 ? 0 : hs.nk_last, K.nk.back());
                for (int mt = 0; mt < hs.mt1; ++mt)
                    for (int gg = 0; gg < 4; ++gg)
                        for (int r = 0; r < 4; ++r) {
                            int fo = 16 * mt + 4 * r + gg;
                            bnode[mt * 16 + gg * 4 + r] = fo < p ? (float)bias1[fo] : 0.f;
                        }
                int n_out = p;
                if (hs.has_exp) {
                    const int s = nd.A2.out;
                    n_out = s;
                    std::vector<int> foff(nd.funcs.size());
                    int eo = 0;
                    for (size_t fi = 0; fi < nd.funcs.size(); ++fi) {
                        foff[fi] = eo;
                        eo += nd.funcs[fi].out_dim(p);
                    }
                    if (eo != nd.A2.in) fail(HG_ERR_DIM, "fused: expansion width %d != second affine input_dim %d", eo, nd.A2.in);
                    std::vector<double> bias2 = nd.A2.b;
                    for (int c = 0; c < nd.A2.in; ++c)
                        for (int o = 0; o < s; ++o) bias2[o] -= nd.A2.a[c] * nd.A2.W[(size_t)c * s + o];
                    float* w2 = wnode + (size_t)a1_blocks * 256;
                    for (int mt1 = 0; mt1 < hs.mt1; ++mt1)
                        for (int fi = 0; fi < hs.nf; ++fi) {
                            const int used = nd.funcs[fi].used(p);
                            hs.mfma_per_tile += (int64_t)hs.nk2[mt1][fi] * hs.mt2;
                            hs.ks2_tile += hs.nk2[mt1][fi];
                            for (int mt2 = 0; mt2 < hs.mt2; ++mt2) {
                                float* blk = w2 + ((size_t)(mt1 * hs.nf + fi) * hs.mt2 + mt2) * 256;
                                for (int lane = 0; lane < 64; ++lane) {
                                    int i = lane & 15, gg = lane >> 4;
                                    int fo = 16 * mt2 + q_of_row(i);
                                    if (fo >= s) continue;
                                    for (int r = 0; r < 4; ++r) {
                                        int fz = 16 * mt1 + 4 * r + gg;
                                        if (fz >= used) continue;
                                        blk[lane * 4 + r] = (float)nd.A2.W[(size_t)(foff[fi] + fz) * s + fo];
                                    }
                                }
                            }
                        }
                    for (int mt = 0; mt < hs.mt2; ++mt)
                        for (int gg = 0; gg < 4; ++gg)
                            for (int r = 0; r < 4; ++r) {
                                int fo = 16 * mt + 4 * r + gg;
                                bnode[hs.mt1 * 16 + mt * 16 + gg * 4 + r] = fo < s ? (float)bias2[fo] : 0.f;
                            }
                }
                node_out.push_back(n_out);
            }
            // Remainder tiles (hg_fused_dev.hpp): when the last tile of BOTH affines holds 1..4 real rows, store its
            // A fragments in 4x4 form for the k_stage REM instantiations.  Only stages that always run on
            // k_stage: not the first two (front kernels read the ordinary form) and more than 4 nodes
            // (k_stage_splitm takes the small ones).
            {
                const int r1 = hs.p_max - 16 * (hs.mt1 - 1), r2 = hs.s_max - 16 * (hs.mt2 - 1);
                hs.rem4 = si >= 1 && hs.has_exp && n > 4 && hs.mt1 == hs.mt2 && (hs.mt1 == 2 || hs.mt1 == 3) && r1 >= 1 && r1 <= 4 &&
                          r2 >= 1 && r2 <= 4 && !opt.no_rem4 && !st.sum_in;
                if (hs.rem4) {
                    auto to4x4 = [](float* blk) {
                        float old[256];
                        std::copy(blk, blk + 256, old);
                        for (int l = 0; l < 64; ++l) {
                            const int src = (l & 48) | ((l & 3) << 2);
                            for (int r = 0; r < 4; ++r) blk[l * 4 + r] = old[src * 4 + r];
                        }
                    };
                    for (int ni = 0; ni < n; ++ni) {
                        float* wnode = hs.afrag.data() + (size_t)ni * hs.node_blocks * 256;
                        for (int kb = 0; kb < hs.kb1; ++kb) to4x4(wnode + ((size_t)kb * hs.mt1 + hs.mt1 - 1) * 256);
                        float* w2 = wnode + (size_t)hs.kb1 * hs.mt1 * 256;
                        for (int b2 = 0; b2 < hs.mt1 * hs.nf; ++b2) to4x4(w2 + ((size_t)b2 * hs.mt2 + hs.mt2 - 1) * 256);
                    }
                    // the 4x4 tiles cost a quarter of the MFMA time of a 16x16 tile
                }
            }
            // Packed remainder tiles: only where this stage always runs on a kernel that writes them (k_stage REM, or the fused
            // front kernel for stage 1) and the next stage always runs on one that decodes them (k_stage: an ordinary layer of
            // more than 16 nodes — not the split-m, chain, product or iGSFA kernels).
            hs.pack_out = false;
            if (hs.rem4 && n % 4 == 0 && !opt.no_pack && si + 1 < fs.size()) {
                const FStage& nx = fs[si + 1];
                bool ok = nx.nodes.size() > 16;
                for (auto& nd : nx.nodes) ok = ok && !nd.is_ig && !nd.has_prod && !nd.has_clip && nd.has_exp;
                hs.pack_out = ok;
            }
            if (hs.pack_out) {
                // which four nodes share a block: order the nodes by the node of the next layer that reads their remainder rows
                // (first reader), so that the children of one parent — and of its neighbour — sit in one block: the parent then
                // reads them as ONE K-block.  Any grouping is correct; this one saves loads.
                const FStage& nx = fs[si + 1];
                std::vector<int> col0(n, 0), reader(n, 1 << 30);
                for (int ni = 1; ni < n; ++ni) col0[ni] = col0[ni - 1] + node_out[ni - 1];
                std::vector<int> owner;           // output column -> node
                for (int ni = 0; ni < n; ++ni) owner.insert(owner.end(), node_out[ni], ni);
                for (size_t pj = 0; pj < nx.nodes.size(); ++pj)
                    for (int c = 0; c < nx.nodes[pj].in_dim; ++c) {
                        const int col = nx.conn[nx.nodes[pj].in_off + c];
                        const int ni = owner[col];
                        if (col - col0[ni] >= 16 * (hs.mto - 1)) reader[ni] = std::min(reader[ni], (int)pj);
                    }
                std::vector<int> order(n);
                for (int ni = 0; ni < n; ++ni) order[ni] = ni;
                std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return reader[a] < reader[b]; });
                hs.pack_slot.assign(n, 0);
                for (int rk = 0; rk < n; ++rk) hs.pack_slot[order[rk]] = rk;
            }
            for (int ni = 0; ni < n; ++ni)
                for (int f = 0; f < node_out[ni]; ++f) {
                    if (hs.pack_out && f >= 16 * (hs.mto - 1)) {
                        cur_blk.push_back(n * (hs.mto - 1) + hs.pack_slot[ni] / 4);
                        cur_q.push_back(4 * (hs.pack_slot[ni] % 4) + (f - 16 * (hs.mto - 1)));
                    } else {
                        cur_blk.push_back(ni * (hs.pack_out ? hs.mto - 1 : hs.mto) + f / 16);
                        cur_q.push_back(f % 16);
                    }
                }
            hs.nb_out = hs.pack_out ? n * (hs.mto - 1) + n / 4 : n * hs.mto;
            prev_packed = hs.pack_out;
            prev_blk.swap(cur_blk);
            prev_q.swap(cur_q);
            prev_nb = hs.nb_out;
            max_nb = std::max(max_nb, hs.nb_out);
            {
                // What the kernels ISSUE per 16-row tile: an affine's tile of <= 4 real rows runs on v_mfma_f32_4x4x1 (512 FLOP, 8 cycles)
                // where the stage has remainder tiles — decided above for k_stage, at run time with the same rule for layer 1 inside the
                // front kernel — every other tile on v_mfma_f32_16x16x4 (2048 FLOP, 32 cycles).  Round 4 counted every tile as 16 x 16.
                const bool front_rem = si == 1 && hs.has_exp && hs.mt1 == 2 && hs.mt2 == 2 && hs.p_max <= 20 && hs.s_max <= 20 && hs.nk2[1][0] <= 1 &&
                                       hs.nk2[1][1] <= 1 && !opt.no_rem4;
                const int rem = (hs.rem4 || front_rem) ? 1 : 0;
                hs.mfma16_tile = hs.ks1_tile * (hs.mt1 - rem) + (hs.has_exp ? hs.ks2_tile * (hs.mt2 - rem) : 0);
                hs.mfma4_tile = rem ? hs.ks1_tile + hs.ks2_tile : 0;
            }
            padded_flops += (hs.mfma16_tile * 2048 + hs.mfma4_tile * 512) / 16;
            std::ostringstream os;
            os << "fused stage " << si << (hs.rem4 ? (hs.pack_out ? " (4x4 remainder tiles, packed four to a block)" : " (4x4 remainder tiles)") : "") << ": " << hs.n_nodes << " nodes, K-blocks " << hs.kb1 << ", tiles " << hs.mt1 << "x" << hs.mt2
               << (hs.sum_in ? " (first affine folded into the layer below's second, plain 16-row tiles only: z = bias + the tiles of " + std::to_string(hs.n_kids) + " children)" : "")
               << ", " << hs.mfma_per_tile << " MFMA/tile (issued: " << hs.mfma16_tile << " x 16x16x4 + " << hs.mfma4_tile << " x 4x4x1), " << hs.afrag.size() * 4 / 1024
               << " KiB weights, out " << hs.nb_out << " blocks/tile";
            hs.name = os.str();
            if (st.sum_in && opt.pair) plan_pairs(st, hs);
        }
        plan_slot_major();
        fuse01 = can_fuse01();
        if (fuse01) {
            stages[0].name += "  [+ stage 1 fused in the same persistent kernel when the input allows 16-byte loads]";
        }
        if (opt.fold01) plan_fold01(fs);
        if (opt.fold01_pack) plan_fold01_pack(fs);
        col_base.resize(out_dim);
        col_of.assign((size_t)std::max(prev_nb, 1) * 16, -1);      // inverse map for k_tail: (output block, feature of the tile) -> caller column
        for (int c = 0; c < out_dim; ++c) {
            int q = prev_q[c];
            col_base[c] = prev_blk[c] * 256 + (q & 3) * 64 + (q >> 2);
            col_of[(size_t)prev_blk[c] * 16 + q] = c;
        }
        for (auto& hs : stages)      // k_tail reads 8 K-block entries at once from a node's first: 8 spare ones behind the last node's
            if (!hs.kb1tab.empty()) hs.kb1tab.resize(hs.kb1tab.size() + 16, 0);
        plan_tail();
        plan_subtree();
        for (auto& hs : stages)      // the front kernels read piece_col as int2 pairs: never an empty table
            if (!hs.chunks.empty()) hs.piece_col.resize(std::max<size_t>(hs.piece_col.size(), 2));
    }

    // Summed links (HostStage::pair_kids).  A hoisted stage whose nodes ALL have exactly two children gets what the layer
    // below needs to store one tile set per node — each node's children in first-read order — and what this stage needs to read it: a
    // K-block table of one child per node and a bias array whose first bias is -0.0f.  Whether a call uses them is the executor's business
    // (both layers on the node-group sweep, the preset shape, enough work); every other kernel family keeps reading kb1tab and bias.
    void plan_pairs(const FStage& st, HostStage& hs) {
        size_t lo = ~(size_t)0, hi = 0;
        for (auto& nd : st.nodes) {
            lo = std::min(lo, nd.kids.size());
            hi = std::max(hi, nd.kids.size());
        }
        if (lo != 2 || hi != 2) {
            hs.name += lo == hi ? "; unpaired: " + std::to_string(lo) + " children per node" : "; unpaired: " + std::to_string(lo) + " to " + std::to_string(hi) + " children per node";
            return;
        }
        const int n = hs.n_nodes;
        hs.pair_kids.reserve((size_t)n * 2);
        for (auto& nd : st.nodes) {
            hs.pair_kids.push_back(nd.kids[0]);
            hs.pair_kids.push_back(nd.kids[1]);
        }
        hs.kb1tab_pre.assign(((size_t)n * hs.mt1 + 8) * 2, 0);
        for (int ni = 0; ni < n; ++ni)
            for (int mt = 0; mt < hs.mt1; ++mt) {
                hs.kb1tab_pre[((size_t)ni * hs.mt1 + mt) * 2] = ni * hs.mt1 + mt;
                hs.kb1tab_pre[((size_t)ni * hs.mt1 + mt) * 2 + 1] = 1;
            }
        hs.bias_pre = hs.bias;
        for (int ni = 0; ni < n; ++ni) std::fill_n(hs.bias_pre.begin() + (size_t)ni * hs.bias_floats, hs.mt1 * 16, -0.0f);
        hs.name += "; paired: the layer below may store (bias + child 0) + child 1 once per node where both layers run the node-group sweep";
    }

    // Stage 0: group consecutive nodes into chunks whose distinct input columns fit the LDS tile,
    // turn each chunk's column set into contiguous runs, and record for every node input position
    // its word offset inside the staged row.
    void plan_stage0_inputs(const FStage& st, HostStage& hs) {
        const int n = (int)st.nodes.size();
        int kb1 = 0, max_in = 0;
        for (auto& nd : st.nodes) {
            kb1 = std::max(kb1, (nd.in_dim + 15) / 16);
            max_in = std::max(max_in, nd.in_dim);
        }
        // K-slot assignment inside a block of 16 input positions: slot (r, g) <- position 4r+g, or the
        // transposed 4g+r when that makes the four k-steps of a lane contiguous in the input row
        // (e.g. 4-pixel-wide receptive fields: one ds_read_b128 per fragment instead of four b32)
        s0_transpose = true;
        for (auto& nd : st.nodes) {
            for (int c = 0; c < nd.in_dim && s0_transpose; c += 4)
                for (int r = 1; r < 4 && c + r < nd.in_dim; ++r)
                    if (st.conn[nd.in_off + c + r] != st.conn[nd.in_off + c] + r) s0_transpose = false;
            if (nd.in_dim % 4) s0_transpose = false;
        }
        const int col_budget = std::max(kStage0ChunkCols, (max_in + 3) / 4 * 4);
        if (col_budget > 2048) fail(HG_ERR_FORMAT, "fused: first-layer node with %d inputs", max_in);
        hs.koff.assign((size_t)n * kb1 * 16, -1);
        hs.kmean.assign((size_t)n * kb1 * 16, 0.f);
        int max_cols = 0, ni = 0;
        bool vec_ok = true, contig = true;
        while (ni < n) {
            std::vector<int32_t> cols;
            int n1 = ni;
            while (n1 < n) {
                std::vector<int32_t> c2 = cols;
                const FNode& nd = st.nodes[n1];
                for (int c = 0; c < nd.in_dim; ++c) c2.push_back(st.conn[nd.in_off + c]);
                std::sort(c2.begin(), c2.end());
                c2.erase(std::unique(c2.begin(), c2.end()), c2.end());
                if ((int)c2.size() > col_budget && n1 > ni) break;
                cols.swap(c2);
                ++n1;
            }
            DChunk ck{ni, n1 - ni, (int)hs.runs.size(), 0, 0, (int)hs.piece_col.size() / 2, 0, 0};
            std::map<int32_t, int32_t> lds_of;
            // Four short runs (4-pixel-high fields: run = pixel row = lane group g of the transposed K slots) pack
            // into 128 words: a ds_read_b128 serves lanes in four 16-lane groups that each mix HALF of lane group
            // g = 0 with half of g = 1 (or g = 2 with g = 3; MI355X_MICROARCH.md §LDS), so only those pairs have to
            // agree modulo the 64-word bank row: offsets 0, 64, 32, 96.  Half the LDS of one-run-per-bank-row.
            int n_runs = 0, max_len = 0;
            for (size_t i = 0; i < cols.size();) {
                size_t k = i + 1;
                while (k < cols.size() && cols[k] == cols[k - 1] + 1) ++k;
                ++n_runs;
                max_len = std::max(max_len, (int)(k - i));
                i = k;
            }
            const bool packed4 = s0_transpose && n_runs == 4 && max_len <= 32;
            static const int packed_off[4] = {0, 64, 32, 96};
            int off = 0, run_i = 0, hi = 0;
            for (size_t i = 0; i < cols.size(); ++run_i) {
                size_t k = i + 1;
                while (k < cols.size() && cols[k] == cols[k - 1] + 1) ++k;
                const int len = (int)(k - i);
                // otherwise every run starts on a 64-word (256 B = one LDS bank row) boundary: the four lane
                // groups of a ds_read_b128 then differ only by multiples of the bank row and the 16
                // sub-images of a group (stride == 4 mod 64) take 16 distinct 16-byte slots
                off = packed4 ? packed_off[run_i] : (off + 63) / 64 * 64;
                hs.runs.push_back(DRun{cols[i], len, off, 0});
                if (cols[i] % 4 || len % 4) vec_ok = false;
                for (size_t m = i; m < k; ++m) lds_of[cols[m]] = off + (int)(m - i);
                for (int pc = 0; pc + 3 < len; pc += 4) {
                    hs.piece_col.push_back(cols[i] + pc);
                    hs.piece_col.push_back(off + pc);
                    ++ck.n_pieces;
                }
                off += len;
                hi = std::max(hi, off);
                i = k;
                ++ck.run_count;
            }
            off = hi;
            ck.n_cols = off;
            max_cols = std::max(max_cols, off);
            for (int k = ni; k < n1; ++k) {
                const FNode& nd = st.nodes[k];
                for (int kb = 0; kb < kb1; ++kb)
                    for (int g = 0; g < 4; ++g)
                        for (int r = 0; r < 4; ++r) {
                            int c = kb * 16 + s0_pos(r, g);
                            size_t e = (((size_t)k * kb1 + kb) * 4 + g) * 4 + r;
                            if (c < nd.in_dim) {
                                hs.koff[e] = lds_of[st.conn[nd.in_off + c]];
                                hs.kmean[e] = (float)nd.A1.a[c];
                            }
                        }
            }
            hs.chunks.push_back(ck);
            hs.max_chunk_nodes = std::max(hs.max_chunk_nodes, ck.node_count);
            hs.max_chunk_pieces = std::max(hs.max_chunk_pieces, ck.n_pieces);
            ni = n1;
        }
        // Row stride of the LDS tile: >= max_cols + 1 (last word = the zero column padded k positions
        // read), == 4 (mod 64) words so that the 16 sub-images of a ds_read_b128 lane group land on 16
        // distinct 16-byte slots of the 256-byte bank row (rows stay 16-byte aligned).
        int stride = max_cols + 1;
        while (stride % 64 != 4) ++stride;
        hs.lds_stride = stride;
        for (size_t e = 0; e < hs.koff.size(); e += 4) {
            bool any_pad = false;
            for (int r = 0; r < 4; ++r)
                if (hs.koff[e + r] < 0) {
                    hs.koff[e + r] = stride - 1;
                    any_pad = true;
                }
            if (any_pad || hs.koff[e] % 4) contig = false;
            for (int r = 1; r < 4; ++r)
                if (hs.koff[e + r] != hs.koff[e] + r) contig = false;
        }
        hs.contig4 = contig;
        hs.vec_ok = vec_ok;
        // k_stage01d: every lane group of every node reads four contiguous, 16-byte aligned source columns
        bool direct = contig && vec_ok && s0_transpose && kb1 == 1;
        hs.kcol.assign((size_t)n * 4, 0);
        for (int k = 0; k < n && direct; ++k) {
            const FNode& nd = st.nodes[k];
            if (nd.in_dim != 16) { direct = false; break; }
            for (int g = 0; g < 4; ++g) {
                const int c0 = s0_pos(0, g), col = st.conn[nd.in_off + c0];
                for (int r = 0; r < 4; ++r)
                    if (s0_pos(r, g) != c0 + r || st.conn[nd.in_off + c0 + r] != col + r) direct = false;
                if (col % 4) direct = false;
                hs.kcol[(size_t)k * 4 + g] = col;
            }
        }
        hs.direct_ok = direct;
        if (!direct) hs.kcol.clear();
    }

    // First layer of iGSFA nodes: a gather pseudo-stage turns the row-major input into fragment-order
    // blocks (one block per node K-block), after which the iGSFA layer reads blocks like any other.
    void add_gather0(FStage& st, std::vector<int32_t>& prev_blk, std::vector<int32_t>& prev_q, int& prev_nb) {
        stages.emplace_back();
        HostStage& hs = stages.back();
        hs.kind = 1;
        hs.from_x = true;
        const int n = (int)st.nodes.size();
        int KB = 0;
        bool tr = true;
        for (auto& nd : st.nodes) {
            KB = std::max(KB, (nd.in_dim + 15) / 16);
            for (int c = 0; c < nd.in_dim && tr; c += 4)
                for (int r = 1; r < 4 && c + r < nd.in_dim; ++r)
                    if (st.conn[nd.in_off + c + r] != st.conn[nd.in_off + c] + r) tr = false;
            if (nd.in_dim % 4) tr = false;
        }
        hs.n_nodes = n;
        hs.kb1 = KB;
        hs.nb_out = n * KB;
        hs.gcol.assign((size_t)n * KB * 16, -1);
        const int in_w = (int)st.conn.size();
        prev_blk.assign(in_w, 0);
        prev_q.assign(in_w, 0);
        for (int ni = 0; ni < n; ++ni) {
            const FNode& nd = st.nodes[ni];
            for (int c = 0; c < nd.in_dim; ++c) {
                const int kb = c / 16, pp = c % 16;
                const int q = tr ? 4 * (pp % 4) + pp / 4 : pp;     // slot q = 4r + g
                hs.gcol[((size_t)ni * KB + kb) * 16 + (q & 3) * 4 + (q >> 2)] = st.conn[nd.in_off + c];
                prev_blk[nd.in_off + c] = ni * KB + kb;
                prev_q[nd.in_off + c] = q;
            }
        }
        hs.vec_ok = tr;
        for (size_t e4 = 0; e4 < hs.gcol.size() && hs.vec_ok; e4 += 4)
            if (hs.gcol[e4] >= 0 && hs.gcol[e4 + 3] == hs.gcol[e4] + 3 && hs.gcol[e4] % 4) hs.vec_ok = false;
        for (int i = 0; i < in_w; ++i) st.conn[i] = i;
        prev_nb = hs.nb_out;
        max_nb = std::max(max_nb, hs.nb_out);
        std::ostringstream os;
        os << "fused gather: row-major input -> fragment order, " << n << " nodes x " << KB << " K-blocks";
        hs.name = os.str();
    }

    void build_ig_stage(FStage& st, std::vector<int32_t>& prev_blk, std::vector<int32_t>& prev_q, int& prev_nb) {
        stages.emplace_back();
        HostStage& hs = stages.back();
        hs.kind = 2;
        hs.has_exp = true;
        const int n = (int)st.nodes.size();
        hs.n_nodes = n;
        hs.funcs = st.nodes[0].funcs;
        hs.nf = (int)hs.funcs.size();
        hs.ig_has_lr = st.nodes[0].ig_has_lr;
        hs.nb_in = prev_nb;
        int k_max = 0, out_max = 0;
        struct NodeK {
            std::vector<int> src, nk, pos;   // per K-block: source block, k-steps; per slot: input position or -1
        };
        std::vector<NodeK> nks(n);
        for (int ni = 0; ni < n; ++ni) {
            FNode& nd = st.nodes[ni];
            if (nd.ig_has_lr != hs.ig_has_lr) fail(HG_ERR_FORMAT, "fused: iGSFA nodes of one layer differ in reconstruct_with_sfa");
            k_max = std::max(k_max, nd.ig_k);
            out_max = std::max(out_max, nd.out_dim);
            NodeK& K = nks[ni];
            std::map<int, int> blk_index;
            for (int c = 0; c < nd.in_dim; ++c) {
                const int pc = st.conn[nd.in_off + c];
                const int blk = prev_blk[pc], q = prev_q[pc];
                auto it = blk_index.find(blk);
                int kb;
                if (it == blk_index.end()) {
                    kb = (int)K.src.size();
                    blk_index[blk] = kb;
                    K.src.push_back(blk);
                    K.nk.push_back(0);
                    for (int qq = 0; qq < 16; ++qq) K.pos.push_back(-1);
                } else {
                    kb = it->second;
                }
                if (K.pos[kb * 16 + q] >= 0) fail(HG_ERR_FORMAT, "fused: iGSFA node reads one input column twice");
                K.pos[kb * 16 + q] = c;
                K.nk[kb] = std::max(K.nk[kb], q / 4 + 1);
            }
            hs.kb1 = std::max(hs.kb1, (int)K.src.size());
        }
        if (hs.kb1 > 8) fail(HG_ERR_FORMAT, "fused: iGSFA node input spans more than 8 source blocks");
        // folded form (see igsfa_affine): one GEMM from the expanded input to all output tiles
        std::vector<Aff> folded_a2(n);
        bool folded = true;
        for (int ni = 0; ni < n && folded; ++ni) folded = igsfa_affine(st.nodes[ni], folded_a2[ni], opt.ig_nofold);
        hs.ig_folded = folded;
        if (folded) hs.ig_has_lr = false;
        const int KB = hs.kb1, MO = (out_max + 15) / 16, MS = folded ? MO : (k_max + 15) / 16, nf = hs.nf;
        hs.mt1 = MS;
        hs.mt2 = MO;
        hs.mto = MO;
        for (int ms = 0; ms < MS; ++ms) hs.ig_nks[ms] = (std::min(16, k_max - 16 * ms) + 3) / 4;
        hs.node_blocks = folded ? nf * KB * MO : nf * KB * MS + KB * MS + KB * MO;
        hs.bias_floats = MO * 16 + 2 * KB * 16;
        if ((size_t)hs.node_blocks * 1024 + (size_t)hs.bias_floats * 4 + (size_t)KB * 8 > 150 * 1024)
            fail(HG_ERR_FORMAT, "fused: one iGSFA node needs %d KiB of weight fragments, more than a workgroup's LDS", hs.node_blocks);
        hs.afrag.assign((size_t)n * hs.node_blocks * 256, 0.f);
        hs.bias.assign((size_t)n * hs.bias_floats, 0.f);
        hs.kb1tab.assign((size_t)n * KB * 2, 0);
        std::vector<int32_t> cur_blk, cur_q;
        for (int ni = 0; ni < n; ++ni) {
            FNode& nd = st.nodes[ni];
            NodeK& K = nks[ni];
            const int d = nd.in_dim, k = nd.ig_k, Q = nd.ig_pca.out;
            if (nd.ig_sfa.out != k || nd.ig_pca.in != d || k + Q != nd.out_dim) fail(HG_ERR_DIM, "fused: iGSFA node dimensions");
            std::vector<int> foff(nf), used(nf);
            int eo = 0;
            for (int fi = 0; fi < nf; ++fi) {
                foff[fi] = eo;
                used[fi] = nd.funcs[fi].used(d);
                eo += nd.funcs[fi].out_dim(d);
            }
            if (eo != nd.ig_sfa.in) fail(HG_ERR_DIM, "fused: iGSFA expansion width != sfa input_dim");
            float* wn = hs.afrag.data() + (size_t)ni * hs.node_blocks * 256;
            float* w1 = wn;
            float* w2 = w1 + (size_t)nf * KB * MS * 256;
            float* w3 = w2 + (size_t)KB * MS * 256;
            float* bn = hs.bias.data() + (size_t)ni * hs.bias_floats;
            for (int kb = 0; kb < KB; ++kb) {
                const bool real = kb < (int)K.src.size();
                hs.kb1tab[((size_t)ni * KB + kb) * 2] = real ? K.src[kb] : K.src[0];
                hs.kb1tab[((size_t)ni * KB + kb) * 2 + 1] = real ? K.nk[kb] : 0;
                if (!real) continue;
                hs.mfma_per_tile += (int64_t)K.nk[kb] * (folded ? nf * MO : nf * MS + MO);
                for (int ms = 0; ms < MS && hs.ig_has_lr; ++ms) hs.mfma_per_tile += hs.ig_nks[ms];
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = lane & 15, gg = lane >> 4;
                    for (int r = 0; r < 4; ++r) {
                        const int cs = K.pos[kb * 16 + 4 * r + gg];           // input position of this k-slot
                        if (folded) {     // rows = all output features, k-slots = expanded input positions
                            const Aff& F = folded_a2[ni];
                            for (int fi = 0; fi < nf; ++fi)
                                for (int mo = 0; mo < MO; ++mo) {
                                    const int f = 16 * mo + q_of_row(i);
                                    if (f < k + Q && cs >= 0 && cs < used[fi])
                                        w1[(((size_t)fi * KB + kb) * MO + mo) * 256 + lane * 4 + r] =
                                            (float)F.W[(size_t)(foff[fi] + cs) * (k + Q) + f];
                                }
                            continue;
                        }
                        // W1: rows = slow features, k-slots = expanded input positions
                        for (int fi = 0; fi < nf; ++fi)
                            for (int ms = 0; ms < MS; ++ms) {
                                const int fs = 16 * ms + q_of_row(i);
                                if (fs < k && cs >= 0 && cs < used[fi])
                                    w1[(((size_t)fi * KB + kb) * MS + ms) * 256 + lane * 4 + r] =
                                        (float)nd.ig_sfa.W[(size_t)(foff[fi] + cs) * k + fs];
                            }
                        // W3: rows = output features k.., k-slots = residual positions
                        for (int mo = 0; mo < MO; ++mo) {
                            const int f = 16 * mo + q_of_row(i);
                            if (f >= k && f < k + Q && cs >= 0)
                                w3[((size_t)kb * MO + mo) * 256 + lane * 4 + r] = (float)nd.ig_pca.W[(size_t)cs * Q + (f - k)];
                        }
                        // W2: rows = residual positions of this block, k-slots = slow features of tile ms
                        const int crow = K.pos[kb * 16 + q_of_row(i)];
                        if (hs.ig_has_lr && crow >= 0)
                            for (int ms = 0; ms < MS; ++ms) {
                                const int fs = 16 * ms + 4 * r + gg;
                                if (fs < k) w2[((size_t)kb * MS + ms) * 256 + lane * 4 + r] = (float)(-nd.ig_lr.W[(size_t)fs * d + crow]);
                            }
                    }
                }
                for (int gg = 0; gg < 4; ++gg)
                    for (int r = 0; r < 4; ++r) {
                        const int c = K.pos[kb * 16 + 4 * r + gg];
                        if (c < 0) continue;
                        double brv = 0;
                        if (hs.ig_has_lr) {
                            brv = -nd.ig_lr.b[c];
                            for (int fs = 0; fs < k; ++fs) brv += nd.ig_lr.a[fs] * nd.ig_lr.W[(size_t)fs * d + c];
                        }
                        bn[MO * 16 + kb * 16 + gg * 4 + r] = (float)brv;
                        bn[MO * 16 + KB * 16 + kb * 16 + gg * 4 + r] = (float)nd.ig_mean[c];
                    }
            }
            for (int mo = 0; mo < MO; ++mo)
                for (int gg = 0; gg < 4; ++gg)
                    for (int r = 0; r < 4; ++r) {
                        const int f = 16 * mo + 4 * r + gg;
                        double v = 0;
                        if (folded) {
                            if (f < k + Q) v = folded_a2[ni].b[f];
                        } else if (f < k) {
                            v = nd.ig_sfa.b[f];
                            for (int e = 0; e < nd.ig_sfa.in; ++e) v -= nd.ig_sfa.a[e] * nd.ig_sfa.W[(size_t)e * k + f];
                        } else if (f < k + Q) {
                            v = nd.ig_pca.b[f - k];
                            for (int c = 0; c < d; ++c) v -= nd.ig_pca.a[c] * nd.ig_pca.W[(size_t)c * Q + (f - k)];
                        }
                        bn[mo * 16 + gg * 4 + r] = (float)v;
                    }
            for (int f = 0; f < nd.out_dim; ++f) {
                cur_blk.push_back(ni * MO + f / 16);
                cur_q.push_back(f % 16);
            }
        }
        hs.nb_out = n * MO;
        prev_blk.swap(cur_blk);
        prev_q.swap(cur_q);
        prev_nb = hs.nb_out;
        max_nb = std::max(max_nb, hs.nb_out);
        padded_flops += hs.mfma_per_tile * 2048 / 16;
        std::ostringstream os;
        os << "fused iGSFA stage" << (folded ? " (folded to one GEMM)" : "") << ": " << n << " nodes, K-blocks " << KB << ", slow tiles " << MS << ", out tiles " << MO << ", "
           << hs.mfma_per_tile << " MFMA/tile, " << hs.afrag.size() * 4 / 1024 << " KiB weights";
        hs.name = os.str();
    }

    // Layer whose expansion holds cross-column products or is followed by a CutoffNode (k_stage_prod).  GEMM 1 as in any
    // stage > 0; the expanded input is described column by column for the WIDEST node of the layer, 16 columns per K-block
    // of GEMM 2; a narrower node's weights are scattered into that column order (columns it lacks get zero rows).
    void build_prod_stage(FStage& st, std::vector<int32_t>& prev_blk, std::vector<int32_t>& prev_q, int& prev_nb, int si) {
        stages.emplace_back();
        HostStage& hs = stages.back();
        hs.kind = 3;
        hs.has_exp = true;
        const int n = (int)st.nodes.size();
        hs.n_nodes = n;
        const std::vector<ExpFunc> all = st.nodes[0].funcs;
        const int nf_all = (int)all.size();
        std::vector<int> elem_of(nf_all, -1);          // function -> index among the element-wise ones
        for (int fi = 0; fi < nf_all; ++fi)
            if (all[fi].kind <= E_SIGNED_POW) {
                elem_of[fi] = (int)hs.funcs.size();
                hs.funcs.push_back(all[fi]);
            }
        hs.nf = (int)hs.funcs.size();
        if (hs.nf > kMaxFuncs) fail(HG_ERR_FORMAT, "fused: more than 4 element-wise expansion functions");
        hs.has_clip = st.nodes[0].has_clip;
        hs.clip_lo = (float)st.nodes[0].clip_lo;
        hs.clip_hi = (float)st.nodes[0].clip_hi;
        hs.nb_in = prev_nb;
        for (auto& nd : st.nodes) {
            if (!nd.has_exp) fail(HG_ERR_FORMAT, "fused: linear node in a layer with product expansions");
            hs.p_max = std::max(hs.p_max, nd.A1.out);
            hs.s_max = std::max(hs.s_max, nd.A2.out);
        }
        hs.mt1 = (hs.p_max + 15) / 16;
        hs.mt2 = (hs.s_max + 15) / 16;
        hs.mto = hs.mt2;
        for (int mt1 = 0; mt1 < hs.mt1; ++mt1)
            for (int fi = 0; fi < hs.nf; ++fi) {
                const int valid = std::max(0, std::min(16, hs.funcs[fi].used(hs.p_max) - 16 * mt1));
                hs.nk2[mt1][fi] = (uint8_t)((valid + 3) / 4);
            }
        // product columns of a node of width p: (function, i, k) in the order GeneralExpansionNode stacks them
        struct Col { int fi, i, k; };
        auto products = [&](int p) {
            std::vector<Col> cols;
            for (int fi = 0; fi < nf_all; ++fi) {
                const ExpFunc& f = all[fi];
                const int u = f.used(p);
                if (f.kind == E_QUADRATIC) { for (int i = 0; i < u; ++i) for (int k = i; k < u; ++k) cols.push_back({fi, i, k}); }
                else if (f.kind == E_PAIR_ADJ) for (int i = 0; i + (int)f.k < u; ++i) cols.push_back({fi, i, i + (int)f.k});
                else if (f.kind == E_PAIR_BAND)
                    for (int off = 0; off < (int)f.k; ++off) for (int i = 0; i + off < u; ++i) cols.push_back({fi, i, i + off});
            }
            return cols;
        };
        const std::vector<Col> cmax = products(hs.p_max);
        const int E = (int)cmax.size();
        hs.neb = (E + 15) / 16;
        hs.nk_last = hs.neb ? (std::min(16, E - 16 * (hs.neb - 1)) + 3) / 4 : 0;
        hs.etab.assign((size_t)std::max(hs.neb, 1) * 32, 0);
        for (int c = 0; c < E; ++c) {
            hs.etab[2 * c] = (int32_t)(0x80000000u | (uint32_t)(cmax[c].i * 64));     // byte offset of feature i in [feature][16 sub-images]
            hs.etab[2 * c + 1] = cmax[c].k * 64;
        }
        // K-blocks of GEMM 1
        struct NodeK {
            std::vector<int> src, nk;
            std::vector<std::vector<int>> kpos;
        };
        std::vector<NodeK> nks(n);
        for (int ni = 0; ni < n; ++ni) {
            FNode& nd = st.nodes[ni];
            NodeK& K = nks[ni];
            std::map<int, int> blk_index;
            for (int c = 0; c < nd.in_dim; ++c) {
                const int pc = st.conn[nd.in_off + c], blk = prev_blk[pc], q = prev_q[pc];
                auto it = blk_index.find(blk);
                int kb;
                if (it == blk_index.end()) {
                    kb = (int)K.src.size();
                    blk_index[blk] = kb;
                    K.src.push_back(blk);
                    K.nk.push_back(0);
                    for (int qq = 0; qq < 16; ++qq) K.kpos.emplace_back();
                } else {
                    kb = it->second;
                }
                K.kpos[kb * 16 + q].push_back(c);
                K.nk[kb] = std::max(K.nk[kb], q / 4 + 1);
            }
            hs.kb1 = std::max(hs.kb1, (int)K.src.size());
        }
        hs.node_blocks = hs.kb1 * hs.mt1 + (hs.mt1 * hs.nf + hs.neb) * hs.mt2;
        hs.bias_floats = (hs.mt1 + hs.mt2) * 16;
        if ((size_t)hs.node_blocks * 1024 + (size_t)hs.bias_floats * 4 + (size_t)hs.kb1 * 8 + (size_t)hs.neb * 128 + (size_t)4 * hs.mt1 * 1024 > 150 * 1024)
            fail(HG_ERR_FORMAT, "fused: one node needs %d KiB of weight fragments (%d product columns), more than a workgroup's LDS", hs.node_blocks, E);
        hs.afrag.assign((size_t)n * hs.node_blocks * 256, 0.f);
        hs.bias.assign((size_t)n * hs.bias_floats, 0.f);
        hs.kb1tab.assign((size_t)n * hs.kb1 * 2, 0);
        std::vector<int32_t> cur_blk, cur_q;
        for (int ni = 0; ni < n; ++ni) {
            FNode& nd = st.nodes[ni];
            NodeK& K = nks[ni];
            const int p = nd.A1.out, sdim = nd.A2.out;
            float* wnode = hs.afrag.data() + (size_t)ni * hs.node_blocks * 256;
            float* bnode = hs.bias.data() + (size_t)ni * hs.bias_floats;
            std::vector<double> bias1 = nd.A1.b;
            for (int c = 0; c < nd.in_dim; ++c)
                for (int o = 0; o < p; ++o) bias1[o] -= nd.A1.a[c] * nd.A1.W[(size_t)c * p + o];
            for (int kb = 0; kb < hs.kb1; ++kb) {
                const bool real = kb < (int)K.src.size();
                hs.kb1tab[((size_t)ni * hs.kb1 + kb) * 2] = real ? K.src[kb] : K.src[0];
                hs.kb1tab[((size_t)ni * hs.kb1 + kb) * 2 + 1] = real ? K.nk[kb] : 0;
                if (!real) continue;
                hs.mfma_per_tile += (int64_t)K.nk[kb] * hs.mt1;
                for (int mt = 0; mt < hs.mt1; ++mt) {
                    float* blk = wnode + ((size_t)kb * hs.mt1 + mt) * 256;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i = lane & 15, gg = lane >> 4, fo = 16 * mt + q_of_row(i);
                        if (fo >= p) continue;
                        for (int r = 0; r < 4; ++r) {
                            double w = 0;
                            for (int c : K.kpos[kb * 16 + 4 * r + gg]) w += nd.A1.W[(size_t)c * p + fo];
                            blk[lane * 4 + r] = (float)w;
                        }
                    }
                }
            }
            for (int mt = 0; mt < hs.mt1; ++mt)
                for (int gg = 0; gg < 4; ++gg)
                    for (int r = 0; r < 4; ++r) {
                        const int fo = 16 * mt + 4 * r + gg;
                        bnode[mt * 16 + gg * 4 + r] = fo < p ? (float)bias1[fo] : 0.f;
                    }
            // rows of this node's W2: its own expanded columns in GeneralExpansionNode order
            std::vector<int> foff(nf_all);
            int eo = 0;
            for (int fi = 0; fi < nf_all; ++fi) {
                foff[fi] = eo;
                eo += all[fi].out_dim(p);
            }
            if (eo != nd.A2.in) fail(HG_ERR_DIM, "fused: expansion width %d != second affine input_dim %d", eo, nd.A2.in);
            std::map<std::tuple<int, int, int>, int> row_of;      // product (function, i, k) -> row
            {
                const std::vector<Col> cn = products(p);
                std::vector<int> cnt(nf_all, 0);
                for (auto& c : cn) row_of[std::make_tuple(c.fi, c.i, c.k)] = foff[c.fi] + cnt[c.fi]++;
            }
            std::vector<double> bias2 = nd.A2.b;
            for (int c = 0; c < nd.A2.in; ++c)
                for (int o = 0; o < sdim; ++o) bias2[o] -= nd.A2.a[c] * nd.A2.W[(size_t)c * sdim + o];
            float* w2 = wnode + (size_t)hs.kb1 * hs.mt1 * 256;
            for (int mt1 = 0; mt1 < hs.mt1; ++mt1)
                for (int fa = 0; fa < nf_all; ++fa) {
                    const int fi = elem_of[fa];
                    if (fi < 0) continue;
                    const int used = all[fa].used(p);
                    hs.mfma_per_tile += (int64_t)hs.nk2[mt1][fi] * hs.mt2;
                    for (int mt2 = 0; mt2 < hs.mt2; ++mt2) {
                        float* blk = w2 + ((size_t)(mt1 * hs.nf + fi) * hs.mt2 + mt2) * 256;
                        for (int lane = 0; lane < 64; ++lane) {
                            const int i = lane & 15, gg = lane >> 4, fo = 16 * mt2 + q_of_row(i);
                            if (fo >= sdim) continue;
                            for (int r = 0; r < 4; ++r) {
                                const int fz = 16 * mt1 + 4 * r + gg;
                                if (fz >= used) continue;
                                blk[lane * 4 + r] = (float)nd.A2.W[(size_t)(foff[fa] + fz) * sdim + fo];
                            }
                        }
                    }
                }
            float* wp = w2 + (size_t)hs.mt1 * hs.nf * hs.mt2 * 256;
            for (int eb = 0; eb < hs.neb; ++eb) {
                hs.mfma_per_tile += (int64_t)(eb + 1 < hs.neb ? 4 : hs.nk_last) * hs.mt2;
                for (int mt2 = 0; mt2 < hs.mt2; ++mt2) {
                    float* blk = wp + ((size_t)eb * hs.mt2 + mt2) * 256;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i = lane & 15, gg = lane >> 4, fo = 16 * mt2 + q_of_row(i);
                        if (fo >= sdim) continue;
                        for (int r = 0; r < 4; ++r) {
                            const int c = 16 * eb + 4 * r + gg;
                            if (c >= E) continue;
                            auto it = row_of.find(std::make_tuple(cmax[c].fi, cmax[c].i, cmax[c].k));
                            if (it == row_of.end()) continue;        // a column only wider nodes have
                            blk[lane * 4 + r] = (float)nd.A2.W[(size_t)it->second * sdim + fo];
                        }
                    }
                }
            }
            for (int mt = 0; mt < hs.mt2; ++mt)
                for (int gg = 0; gg < 4; ++gg)
                    for (int r = 0; r < 4; ++r) {
                        const int fo = 16 * mt + 4 * r + gg;
                        bnode[hs.mt1 * 16 + mt * 16 + gg * 4 + r] = fo < sdim ? (float)bias2[fo] : 0.f;
                    }
            for (int f = 0; f < sdim; ++f) {
                cur_blk.push_back(ni * hs.mto + f / 16);
                cur_q.push_back(f % 16);
            }
        }
        hs.nb_out = n * hs.mto;
        prev_blk.swap(cur_blk);
        prev_q.swap(cur_q);
        prev_nb = hs.nb_out;
        max_nb = std::max(max_nb, hs.nb_out);
        padded_flops += hs.mfma_per_tile * 2048 / 16;
        std::ostringstream os;
        os << "fused stage " << si << " (table-driven expansion: products" << (hs.has_clip ? ", clip" : "") << "): " << n << " nodes, K-blocks " << hs.kb1
           << ", tiles " << hs.mt1 << "x" << hs.mt2 << ", " << hs.nf << " element-wise functions, " << E << " product columns in " << hs.neb
           << " K-blocks, " << hs.mfma_per_tile << " MFMA/tile, " << hs.afrag.size() * 4 / 1024 << " KiB weights";
        hs.name = os.str();
    }

    // The suffix of the stage list that k_tail runs as one launch: ordinary layers (no remainder / packed tiles, K-blocks of the
    // second affine within one load batch) whose widest one needs at most 16 waves — the 4-2-1 nodes at the top of the preset
    // networks — and whose LDS tiles fit; the last layer always qualifies on its own when it is ordinary (then the launch is
    // k_stage_splitm's work plus the row-major store).
    // Slot-major packed blocks (StageParams::pack_soa) between a producer that packs and a consumer whose large-batch kernel is the
    // whole-visit-prefetch instantiation with remainder tiles (k_stage<.., REM, KBF = 3, .., PK>): every node of the consumer must
    // read exactly one packed block, at the same position of its K-block list, with at most two k-steps.  The consumer's A
    // fragments of that block are shifted so that its k-steps come first, and the table entry carries the first slot instead of
    // a first k-step (load_kblock_soa).  Same products in the same order as the lane-major form.  HIGSFA_NO_SOA=1: off.
    void plan_slot_major() {
        if (opt.no_soa) return;
        for (size_t si = 0; si + 1 < stages.size(); ++si) {
            HostStage& pr = stages[si];
            HostStage& co = stages[si + 1];
            if (!pr.pack_out || co.kind != 0 || !co.rem4 || co.kb1 != 3 || co.mt1 != co.mt2 || (co.mt1 != 2 && co.mt1 != 3)) continue;
            const int base = pr.n_nodes * (pr.mto - 1);
            int pk = -1;
            bool ok = true;
            for (int ni = 0; ni < co.n_nodes && ok; ++ni) {
                int seen = 0;
                for (int kb = 0; kb < co.kb1; ++kb) {
                    const int src = co.kb1tab[((size_t)ni * co.kb1 + kb) * 2], y = co.kb1tab[((size_t)ni * co.kb1 + kb) * 2 + 1];
                    if (src < base) continue;
                    const int nk = y & 255, r0 = y >> 8;
                    ++seen;
                    if (nk == 0 || nk - r0 > 2 || (pk >= 0 && pk != kb)) ok = false;
                    pk = kb;
                }
                if (seen != 1) ok = false;
            }
            if (!ok || pk != 1) continue;      // (instantiated for position 1 of 3: two children with one remainder block between their full tiles)
            for (int ni = 0; ni < co.n_nodes; ++ni) {
                int32_t& y = co.kb1tab[((size_t)ni * co.kb1 + pk) * 2 + 1];
                const int nk = y & 255, r0 = y >> 8;
                float* wnode = co.afrag.data() + (size_t)ni * co.node_blocks * 256;
                for (int mt = 0; mt < co.mt1; ++mt) {
                    float* blk = wnode + ((size_t)pk * co.mt1 + mt) * 256;
                    for (int lane = 0; lane < 64; ++lane) {
                        float v[4] = {0.f, 0.f, 0.f, 0.f};
                        for (int r = r0; r < nk; ++r) v[r - r0] = blk[lane * 4 + r];
                        for (int r = 0; r < 4; ++r) blk[lane * 4 + r] = v[r];
                    }
                }
                y = (nk - r0) | (r0 << 16);
            }
            pr.pack_soa = true;
            co.pack_in = base;
            co.pk_kbi = pk;
            pr.name += "  [packed blocks slot-major]";
        }
    }

    void plan_tail() {
        tail_begin = -1;
        if (opt.tail_max <= 0) return;
        const int ns = (int)stages.size();
        int b = ns;
        int act_blocks = 0, e_blocks = 0;
        while (b > (fuse01 ? 2 : 1) && ns - b < opt.tail_max) {
            const HostStage& s = stages[b - 1];
            // (slot-major packed input — pk_kbi, pack_in — only follows rem4 today; k_tail would misread it, so it is refused on its own)
            if (s.kind != 0 || s.from_x || s.rem4 || s.pack_out || s.pk_kbi >= 0 || s.pack_in != INT32_MAX || s.nf > kMaxFuncs) break;
            if (s.has_exp && s.mt1 * s.nf > 8) break;
            const int waves = s.n_nodes * (s.has_exp ? std::max(s.mt1, s.mt2) : s.mt1);
            if (waves > 16) break;
            const int act = b - 1 < ns - 1 ? std::max(act_blocks, s.nb_out) : act_blocks;      // the last layer's output goes to y
            const int eb = std::max(e_blocks, s.has_exp ? s.n_nodes * s.nf * s.mt1 : 0);
            if (((size_t)2 * act + eb) * 1024 > 150 * 1024) break;
            act_blocks = act;
            e_blocks = eb;
            --b;
        }
        if (b == ns) return;
        tail_begin = b;
        tail_act_blocks = act_blocks;
        tail_e_blocks = e_blocks;
        for (int i = b; i < ns; ++i)
            stages[i].name += i == b ? (ns - b > 1 ? "  [this and the layers above: ONE launch, activations in LDS, writes the caller's rows]"
                                                    : "  [writes the caller's rows: no unpack pass]")
                                      : "  [in the top-of-hierarchy launch]";
    }

    // Layers below the top that fall into independent sub-trees (k_subtree, hg_fused_tail.hip): runs of two or three ordinary
    // layers under the top-of-hierarchy launch of a short batch, if the nodes each root (node of a run's last layer) draws on,
    // layer by layer, are as many for every root and shared with no other root.
    void plan_subtree() {
        sub_runs.clear();
        if (opt.subtree_max_tiles <= 0) return;
        const int ns = (int)stages.size();
        // (the layer under a short batch's k_tail launch runs alone: tail_start)
        const int end = tail_begin < 0 ? ns : (ns - tail_begin >= 3 ? tail_begin + 1 : tail_begin);
        // Two alternative sets of runs, each taken from the top down, a run ending where the one above begins.  Set 0 starts right under
        // the top launch (U11L-128: layers 6-8 as 4 sub-trees of 4 + 2 + 1 nodes, then layers 3-5 as 32 sub-trees; layers 0-2 pack their
        // remainder tiles and stay per-layer launches), set 1 one layer lower (layers 5-7 as 8 sub-trees).  A call takes the set whose
        // usable runs (sub_run_pays) cover more layers and, if equal, have more sub-trees (pick_sub_set): set 1 for 130 .. 512 rows,
        // where it is 2 us faster per call than set 0's four sub-trees (profiles/r05_subtree_call_times.txt).
        plan_subtree_set(end, 0);
        if (!sub_runs.empty()) plan_subtree_set(end - 1, 1);
    }

    void plan_subtree_set(int end, int set) {
        while (end - 1 >= 2) {
            const int last = end - 1;
            const int k = stages[last].n_nodes;
            int b = last + 1, act_blocks = 0, e_blocks = 0;
            std::vector<std::vector<int32_t>> members(kMaxTail), tabs(kMaxTail);      // by distance from `last`
            while (k >= 4 && b > (fuse01 ? 2 : 1) && last + 1 - b < kMaxTail) {
                const HostStage& s = stages[b - 1];
                if (s.kind != 0 || s.from_x || s.rem4 || s.pack_out || s.pk_kbi >= 0 || s.pack_in != INT32_MAX || s.nf > kMaxFuncs ||
                    s.n_nodes % k)      // (slot-major packed input: as in plan_tail)
                    break;
                if (s.has_exp && s.mt1 * s.nf > 8) break;
                const int per = s.n_nodes / k;
                if (per * (s.has_exp ? std::max(s.mt1, s.mt2) : s.mt1) > 16) break;
                std::vector<int32_t> mem((size_t)k * per, -1), tab;
                if (b - 1 == last) {
                    for (int j = 0; j < k; ++j) mem[j] = j;
                } else {
                    // nodes of this layer under each root, in the order the layer above first reads them
                    const HostStage& up = stages[b];
                    const std::vector<int32_t>& mup = members[last - b];
                    const int per_up = up.n_nodes / k;
                    std::vector<int32_t> owner(s.n_nodes, -1), pos(s.n_nodes, -1);
                    bool ok = s.nb_out == s.n_nodes * s.mto;
                    tab.assign(up.kb1tab.size(), 0);
                    for (int j = 0; j < k && ok; ++j) {
                        int have = 0;
                        for (int q = 0; q < per_up && ok; ++q) {
                            const int ni = mup[(size_t)j * per_up + q];
                            for (int kb = 0; kb < up.kb1 && ok; ++kb) {
                                const size_t at = ((size_t)ni * up.kb1 + kb) * 2;
                                const int src = up.kb1tab[at];
                                if (src < 0 || src >= s.nb_out) { ok = false; break; }
                                const int sn = src / s.mto;
                                if (owner[sn] < 0) {
                                    if (have == per) { ok = false; break; }
                                    owner[sn] = j;
                                    pos[sn] = have;
                                    mem[(size_t)j * per + have++] = sn;
                                } else if (owner[sn] != j) {
                                    ok = false;
                                    break;
                                }
                                tab[at] = pos[sn] * s.mto + src % s.mto;
                                tab[at + 1] = up.kb1tab[at + 1];
                            }
                        }
                        if (have != per) ok = false;
                    }
                    if (!ok) break;
                }
                const int act = b - 1 < last ? std::max(act_blocks, per * s.mto) : act_blocks;
                const int eb = std::max(e_blocks, s.has_exp ? per * s.nf * s.mt1 : 0);
                if (((size_t)2 * act + eb) * 1024 > 150 * 1024) break;
                act_blocks = act;
                e_blocks = eb;
                members[last - (b - 1)] = std::move(mem);
                if (b - 1 < last) tabs[last - b] = std::move(tab);      // the table of the layer above this one
                --b;
            }
            if (last + 1 - b < 2) {      // no run ends here: this layer stays a launch of its own
                end = last;
                continue;
            }
            SubRun r;
            r.begin = b;
            r.len = last + 1 - b;
            r.n = k;
            r.act_blocks = act_blocks;
            r.e_blocks = e_blocks;
            r.set = set;
            for (int i = b; i <= last; ++i) {
                r.nodes[i - b] = members[last - i];
                if (i > b) r.tab[i - b] = tabs[last - i];
            }
            sub_runs.push_back(std::move(r));
            if (set != 0) {      // (the stage names describe set 0)
                stages[b].name += "  [or, where more layers or more sub-trees can run that way: " + std::to_string(last + 1 - b) + " layers from here as " + std::to_string(k) + " sub-trees]";
                end = b;
                continue;
            }
            for (int i = b; i <= last; ++i) {
                stages[i].name += i == b ? "  [batches of up to " + std::to_string(std::min(opt.subtree_max_tiles, opt.subtree_max_wgs / k) * 16) + " rows: this and the next " +
                                                std::to_string(last - b) + " layer(s) as " + std::to_string(k) + " sub-trees in ONE launch]"
                                          : "  [in the sub-tree launch for short batches]";
            }
            end = b;
        }
    }

    // The link 0 -> 1 (DESIGN.md §3.1 "Hoisted links").  hoist_first_affines leaves it alone: folding it would widen layer 0's stored
    // output.  In the front kernels that output is never stored — a wave holds both children's z0 and feeds them on — so there the
    // fold costs no bytes: with F_c = A2_c A1_q[rows of c, :],
    //     z1_q = bias'_q + sum_c [z0_c, |z0_c|^p] F_c,
    // 16 k-steps of (one 16x16x4 + one 4x4x1) in place of layer 0's second affine (16 x 16x16x4) and layer 1's first (8 + 8).
    // Taken where layers 0 and 1 share the front kernel (fuse01), both expand with exactly (identity, |x|^p) and layer 1 has 4x4
    // remainder tiles; a function of the flow and of no_rem4 alone, so every front variant runs the same arithmetic.  The fold is
    // fold_link's, float64 rounded once.  HostStages 0 and 1 stay whole; the folded fragments and bias are added to stage 1.
    void plan_fold01(const std::vector<FStage>& fs) {
        if (stages.size() < 2) return;
        auto refuse = [&](const std::string& why) {
            fold01_note = "link 0 -> 1 stays as it is: " + why;
            stages[1].name += "  [" + fold01_note + "]";
        };
        if (!fuse01) {
            bool ig = false;
            for (size_t l = 0; l < 2 && l < fs.size(); ++l)
                for (auto& n : fs[l].nodes) ig = ig || n.is_ig || n.was_ig;
            return refuse(ig ? "an iGSFA front end" : "layers 0 and 1 do not share the front kernel");
        }
        const FStage &ch = fs[0], &pa = fs[1];
        HostStage &a = stages[0], &b = stages[1];
        for (auto& n : pa.nodes)
            if (n.was_ig) return refuse("layer 1 is an iGSFA layer (identity first affine, no remainder tiles)");
        for (auto& n : ch.nodes)
            if (n.was_ig) return refuse("layer 0 is an iGSFA layer");
        auto id_pow = [](const HostStage& hs) { return hs.nf == 2 && hs.funcs[0].kind == E_IDENTITY && hs.funcs[1].kind == E_ABS_POW; };
        if (!id_pow(a) || !id_pow(b)) return refuse("both layers must expand with exactly (identity, |x|^p)");
        if (opt.no_rem4) return refuse("4x4 remainder tiles are switched off (HIGSFA_NO_REM4)");
        if (!(b.p_max >= 17 && b.p_max <= 20 && b.s_max >= 17 && b.s_max <= 20 && b.nk2[1][0] <= 1 && b.nk2[1][1] <= 1))
            return refuse("layer 1 has no 4x4 remainder tiles (affines of " + std::to_string(b.p_max) + " and " + std::to_string(b.s_max) + " outputs, not 17..20)");
        const int nc = (int)ch.nodes.size(), np = (int)pa.nodes.size();
        std::vector<int> owner, col0(nc, 0);
        for (int ci = 0; ci < nc; ++ci) {
            col0[ci] = (int)owner.size();
            owner.insert(owner.end(), ch.nodes[ci].out_dim, ci);
        }
        for (int q = 0; q < np; ++q) {      // (can_fuse01 checked the source blocks; the same on columns)
            const FNode& pn = pa.nodes[q];
            if (pn.A1.in != pn.in_dim) return refuse("internal: layer-1 first affine");
            for (int c = 0; c < pn.in_dim; ++c) {
                const int pc = pa.conn[pn.in_off + c];
                if (pc < 0 || pc >= (int)owner.size() || owner[pc] >> 1 != q) return refuse("a layer-1 node reads other nodes than 2n and 2n + 1");
            }
        }
        b.fold_frag.assign((size_t)np * 8 * 256, 0.f);
        b.fold_bias.assign((size_t)np * 32, 0.f);
        auto to4x4 = [](float* blk) {      // as for HostStage::rem4
            float old[256];
            std::copy(blk, blk + 256, old);
            for (int l = 0; l < 64; ++l) {
                const int src = (l & 48) | ((l & 3) << 2);
                for (int r = 0; r < 4; ++r) blk[l * 4 + r] = old[src * 4 + r];
            }
        };
        for (int q = 0; q < np; ++q) {
            const FNode& pn = pa.nodes[q];
            const int P = pn.A1.out;
            const LinkFold lf = fold_link(ch, pa, q, owner, col0, {2 * q, 2 * q + 1});
            for (int sl = 0; sl < 2; ++sl) {
                const FNode& cn = ch.nodes[2 * q + sl];
                const std::vector<double>& F = lf.W[2 * q + sl];
                const int p0 = cn.A1.out;
                int eo = 0;
                for (int fi = 0; fi < 2; ++fi) {
                    const int used = cn.funcs[fi].used(p0);
                    for (int mt = 0; mt < 2; ++mt) {
                        float* blk = b.fold_frag.data() + ((((size_t)q * 2 + sl) * 2 + fi) * 2 + mt) * 256;
                        for (int lane = 0; lane < 64; ++lane) {
                            const int i = lane & 15, gg = lane >> 4;
                            const int fo = 16 * mt + q_of_row(i);
                            if (fo >= P) continue;
                            for (int r = 0; r < 4; ++r) {
                                const int fz = 4 * r + gg;
                                if (fz >= used) continue;
                                blk[lane * 4 + r] = (float)F[(size_t)(eo + fz) * P + fo];
                            }
                        }
                        if (mt == 1) to4x4(blk);
                    }
                    eo += cn.funcs[fi].out_dim(p0);
                }
            }
            for (int mt = 0; mt < 2; ++mt)
                for (int gg = 0; gg < 4; ++gg)
                    for (int r = 0; r < 4; ++r) {
                        const int fo = 16 * mt + 4 * r + gg;
                        b.fold_bias[(size_t)q * 32 + mt * 16 + gg * 4 + r] = fo < P ? (float)lf.bias[fo] : 0.f;
                    }
        }
        // what the front kernels issue now: layer 0 its first affine alone; layer 1 the folded first affine (the k-steps of layer
        // 0's second affine, each one 16x16x4 + one 4x4x1) and its own second
        const int64_t before = padded_flops;
        padded_flops -= (a.mfma16_tile * 2048 + a.mfma4_tile * 512) / 16 + (b.mfma16_tile * 2048 + b.mfma4_tile * 512) / 16;
        a.mfma16_tile = a.ks1_tile;
        a.mfma4_tile = 0;
        b.mfma16_tile = a.ks2_tile + b.ks2_tile;
        b.mfma4_tile = a.ks2_tile + b.ks2_tile;
        padded_flops += (a.mfma16_tile * 2048 + a.mfma4_tile * 512) / 16 + (b.mfma16_tile * 2048 + b.mfma4_tile * 512) / 16;
        fold01_flops = padded_flops - before;
        fold01 = true;
        fold01_note = "link 0 -> 1 folded: layer 0's second affine multiplied into this layer's first, z = bias' + sum over the two children of "
                      "[z0, |z0|^p] (A2 A1[rows of the child, :]) inside the front kernel, which then issues " + std::to_string(a.mfma16_tile) +
                      " x 16x16x4 for layer 0 and " + std::to_string(b.mfma16_tile) + " x 16x16x4 + " + std::to_string(b.mfma4_tile) +
                      " x 4x4x1 for this layer (the counts on the two stage lines are the flow's as given)";
        b.name += "  [" + fold01_note + "]";
    }

    // The folded link's one-row k-steps.  A layer-0 node of 13 outputs keeps feature q in register q / 4 of lane group
    // q % 4, so register 3 holds feature 12 in lane group 0 and padding in the other three: of the folded sum's sixteen k-steps the four
    // of register 3 (per child and function) carry ONE real k-row each.  Packed, the four k-rows are one k-step, k = lane group:
    //     0: child 0, feature 12      1: child 1, feature 12      2: |child 0, feature 12|^p      3: |child 1, feature 12|^p.
    // No cross-lane move: layer 0's first affine itself puts feature 12 where the k-step reads it.  Its fragment and bias get the row
    // of feature 12 (tile row 3) at rows 3 and 11 for an even node and at rows 7 and 15 — not 3 — for an odd one; these rows are
    // padding otherwise.  The kernel adds the two children's registers 3 (each lane group: its value plus an exact +0.0), takes the
    // power of the sum and selects the sum in lane groups 0-1 and the power in 2-3.  Twelve full k-steps and the packed one, 13 in place of
    // 16; the power is evaluated on seven registers of layer 0 instead of eight.  Every value is plan_fold01's (fold_link's float64, rounded once) or layer 0's own float, moved.
    // Taken where the link is folded and every layer-0 node has 13 outputs (4 m + 1 with all four k-steps in use) that both functions expand.
    void plan_fold01_pack(const std::vector<FStage>& fs) {
        if (stages.size() < 2) return;
        auto refuse = [&](const std::string& why) {
            fold01_pack_note = "the link's one-row k-steps stay as they are: " + why;
            stages[1].name += "  [" + fold01_pack_note + "]";
        };
        if (!fold01) return refuse(opt.fold01 ? "the link 0 -> 1 stays as it is" : "the link 0 -> 1 stays as it is (fold01 is off)");
        const FStage& ch = fs[0];
        HostStage &a = stages[0], &b = stages[1];
        for (auto& n : ch.nodes) {
            const int p0 = n.A1.out;
            if (p0 != 13)
                return refuse("a layer-0 node has " + std::to_string(p0) + " outputs, not 13 (4 m + 1: one feature alone in the last register)");
            if (n.funcs[0].used(p0) != p0 || n.funcs[1].used(p0) != p0) return refuse("a layer-0 function does not expand all 13 outputs");
        }
        if (a.kb1 != 1 || a.mt1 != 1 || a.bias_floats < 16) return refuse("internal: layer 0's first affine is not one block");
        const int nc = a.n_nodes, np = b.n_nodes;
        a.fold_a1.assign((size_t)nc * 256, 0.f);
        a.fold_b1.assign((size_t)nc * 16, 0.f);
        for (int ci = 0; ci < nc; ++ci) {
            const float* blk = a.afrag.data() + (size_t)ci * a.node_blocks * 256;      // block 0: the first affine; lane (g, i) holds tile row i
            const float* bias = a.bias.data() + (size_t)ci * a.bias_floats;            // position = tile row
            float* nb = a.fold_a1.data() + (size_t)ci * 256;
            float* bb = a.fold_b1.data() + (size_t)ci * 16;
            std::copy_n(blk, 256, nb);
            std::copy_n(bias, 16, bb);
            for (int row : {7, 11, 15}) {
                bool zero = bias[row] == 0.f;
                for (int g = 0; g < 4; ++g)
                    for (int r = 0; r < 4; ++r) zero = zero && blk[((g * 16 + row) * 4) + r] == 0.f;
                if (!zero) fail(HG_ERR_FORMAT, "internal: a padding row of layer 0's first affine is in use");
            }
            auto copy_row = [&](int to) {
                for (int g = 0; g < 4; ++g)
                    for (int r = 0; r < 4; ++r) nb[((g * 16 + to) * 4) + r] = blk[((g * 16 + 3) * 4) + r];
                bb[to] = bias[3];
            };
            if (ci & 1) {
                copy_row(7);
                copy_row(15);
                for (int g = 0; g < 4; ++g)
                    for (int r = 0; r < 4; ++r) nb[((g * 16 + 3) * 4) + r] = 0.f;
                bb[3] = 0.f;
            } else {
                copy_row(11);
            }
        }
        b.fold_last.assign((size_t)np * 2 * 64, 0.f);
        for (int q = 0; q < np; ++q)
            for (int sl = 0; sl < 2; ++sl)
                for (int fi = 0; fi < 2; ++fi)
                    for (int mt = 0; mt < 2; ++mt) {
                        float* blk = b.fold_frag.data() + ((((size_t)q * 2 + sl) * 2 + fi) * 2 + mt) * 256;
                        const int g = 2 * fi + sl;
                        // lane (0, i), register 3 = k-row (function fi, feature 12) at the tile's row i (4x4 form: at row 4 (i % 4))
                        for (int i = 0; i < 16; ++i) b.fold_last[((size_t)q * 2 + mt) * 64 + g * 16 + i] = blk[i * 4 + 3];
                        for (int lane = 0; lane < 64; ++lane) blk[lane * 4 + 3] = 0.f;
                    }
        const int64_t before = padded_flops;
        b.mfma16_tile -= 3 * (int64_t)np;
        b.mfma4_tile -= 3 * (int64_t)np;
        padded_flops -= (3 * (int64_t)np * 2048 + 3 * (int64_t)np * 512) / 16;
        fold01_flops += padded_flops - before;
        fold01_pack = true;
        fold01_pack_note = "one-row k-steps packed: feature 12 of both children and both functions in ONE k-step behind twelve full ones, this layer then issues " +
                           std::to_string(b.mfma16_tile) + " x 16x16x4 + " + std::to_string(b.mfma4_tile) + " x 4x4x1";
        b.name += "  [" + fold01_pack_note + "]";
    }

    // Layers 0 and 1 can share one kernel when a wave's two layer-0 node slots are exactly the two
    // children of one layer-1 node (see k_stage01p).
    bool can_fuse01() const {
        if (stages.size() < 2) return false;
        const HostStage& a = stages[0];
        const HostStage& b = stages[1];
        if (a.kind != 0 || b.kind != 0 || !a.from_x) return false;
        if (!(a.has_exp && a.mt1 == 1 && a.mt2 == 1 && a.kb1 == 1 && a.nf == 2 && a.contig4 && a.vec_ok)) return false;
        if (a.nk_last != 4 || a.nk2[0][0] != 4 || a.nk2[0][1] != 4) return false;   // the kernel runs all four k-steps unconditionally
        if (a.max_chunk_nodes > 16 || a.max_chunk_pieces > 64) return false;
        for (auto& c : a.chunks)
            if ((c.node_begin & 1) || (c.node_count & 1)) return false;
        if (!(b.has_exp && b.mt1 == 2 && b.mt2 == 2 && b.kb1 == 2 && b.nf == 2 && b.nk2[0][0] == 4 && b.nk2[0][1] == 4)) return false;
        if (b.n_nodes * 2 != a.n_nodes) return false;
        for (int n = 0; n < b.n_nodes; ++n)
            if (b.kb1tab[(size_t)n * 4] != 2 * n || b.kb1tab[(size_t)n * 4 + 2] != 2 * n + 1) return false;
        return true;
    }

    int s0_pos(int r, int g) const { return s0_transpose ? 4 * g + r : 4 * r + g; }
};

}  // namespace

bool FusedPlan::sub_run_pays(const SubRun& r, int n_tiles) const {
    return n_tiles <= opt.subtree_max_tiles && (int64_t)r.n * n_tiles <= opt.subtree_max_wgs;
}

int FusedPlan::pick_sub_set(int n_tiles) const {
    int best = 0, best_cov = -1, best_k = 0;
    for (int set = 0; set < 2; ++set) {
        int cov = 0, mink = 0x7fffffff;
        for (const SubRun& r : sub_runs)
            if (r.set == set && sub_run_pays(r, n_tiles)) {
                cov += r.len;
                mink = std::min(mink, r.n);
            }
        if (cov > best_cov || (cov == best_cov && cov > 0 && mink > best_k)) {
            best = set;
            best_cov = cov;
            best_k = mink;
        }
    }
    return best;
}

int FusedPlan::tail_start(int n_tiles) const {
    const int ns = (int)stages.size();
    bool short_batch = n_tiles < 96;
    const int sub_set = pick_sub_set(n_tiles);
    for (const SubRun& r : sub_runs)      // (a sub-tree run that takes the top launch's first layer: only with HIGSFA_SUBTREE_WGS raised)
        if (r.set == sub_set && r.begin <= tail_begin && tail_begin < r.begin + r.len && sub_run_pays(r, n_tiles)) short_batch = true;
    return (ns - tail_begin >= 3 && short_batch) ? tail_begin + 1 : tail_begin;
}

std::unique_ptr<const FusedPlan> build_fused_plan(const TNode& root, const FusedOptions& opt, std::string* why_not) {
    std::vector<FStage> stages;
    std::string why;
    if (!build_stages(root, stages, why, opt)) {
        if (why_not) *why_not = why;
        return nullptr;
    }
    for (auto& st : stages) {
        const FNode& f0 = st.nodes[0];
        bool table_driven = f0.has_clip;
        for (auto& n : st.nodes) table_driven = table_driven || n.has_prod;
        if (f0.funcs.size() > (size_t)kMaxFuncs && !table_driven) {
            if (why_not) *why_not = "more than 4 expansion functions";
            return nullptr;
        }
        for (auto& n : st.nodes) {
            bool same = n.has_exp == f0.has_exp && n.is_ig == f0.is_ig && n.funcs.size() == f0.funcs.size() && n.has_clip == f0.has_clip &&
                        (!n.has_clip || (n.clip_lo == f0.clip_lo && n.clip_hi == f0.clip_hi));
            for (size_t i = 0; same && i < n.funcs.size(); ++i)
                same = n.funcs[i].kind == f0.funcs[i].kind && n.funcs[i].expo == f0.funcs[i].expo && n.funcs[i].sel == f0.funcs[i].sel &&
                       n.funcs[i].k == f0.funcs[i].k;
            if (!same) {
                if (why_not) *why_not = "nodes of one layer use different expansions";
                return nullptr;
            }
        }
    }
    if (why_not) why_not->clear();
    // hg_info's padded_flops_per_row stays the figure of the flow as given, every layer with its own first affine: where a link
    // is hoisted, the unhoisted plan is built once more for that count alone (load time only)
    int64_t given = -1;
    if (opt.hoist) {
        std::vector<FStage> plain = stages;
        if (!hoist_first_affines(stages, opt).empty()) {
            try {
                FusedOptions o = opt;
                o.hoist = false;
                o.fold01 = false;
                o.fold01_pack = false;
                given = Planner(root, std::move(plain), o).padded_flops;
            } catch (const Error&) {
            }
        }
    }
    try {
        Planner p(root, std::move(stages), opt);
        p.padded_flops_given = given >= 0 ? given : p.padded_flops - p.fold01_flops;
        return std::make_unique<const FusedPlan>(std::move(static_cast<FusedPlan&>(p)));
    } catch (const Error& e) {      // a structure the fused kernels do not cover: generic plan instead
        if (why_not) *why_not = e.what();
        return nullptr;
    }
}

}  // namespace fused
}  // namespace hg
