// graphik_amd/csrc/gik_tables.hip.h -- the host tables of a template, built from the descriptors alone: the slot lists and
// the slot table of the one-unknown-per-lane kernels, the rigid clique and its row numbering, the tables of the workgroup
// and of the node-per-lane kernels, the FK recipe of seed_kernel and the per-node link records of the fixed-anchor solve.
// Host code only, no HIP call: gik_host.hip chooses the path, calls these and uploads what they return;
// tests/host/tables_walk.cpp runs them on the CPU (tests/test_host_tables.py, docs/NOTEBOOK.md 28).  Every word written
// here becomes an LDS or global address in a kernel; the constants and the packings are the kernel headers' own.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "gik_block.hip.h"
#include "gik_npt.hip.h"
#include "gik_wave.hip.h"
#include "graphik_amd.h"

namespace gik {

struct Ent { int j, kind, term, owner; };
typedef std::vector<std::vector<Ent>> SlotLists;
static void sort_slot_lists(SlotLists &ents) {
  for (auto &e : ents)
    std::stable_sort(e.begin(), e.end(), [](const Ent &a, const Ent &b) {
      return a.j != b.j ? a.j < b.j : a.kind < b.kind;
    });
}

// per-node slot lists, in (neighbour, kind) order == the order the reference's edge loop
// (row-major upper-triangle index pairs) accumulates into each row; maxdeg: the busiest node's.  Returns the reason of a
// refusal, empty = fine
static std::string slot_lists(const gik_template_desc *d, SlotLists &ents, int &maxdeg) {
  ents.assign(d->N, {});
  for (int i = 0; i < d->n_terms; ++i) {
    const int a = d->term_i[i], b = d->term_j[i], kind = d->term_kind[i];
    if (a < 0 || b < 0 || a >= d->N || b >= d->N || a == b) return "bad term indices";
    if (kind < GIK_TERM_EQ || kind > GIK_TERM_UPPER) return "bad term kind";
    ents[a].push_back({b, kind, i, a < b ? 1 : 0});
    ents[b].push_back({a, kind, i, b < a ? 1 : 0});
  }
  sort_slot_lists(ents);
  maxdeg = 0;
  for (const auto &e : ents) maxdeg = std::max(maxdeg, (int)e.size());
  return "";
}

// the slot table of the one-unknown-per-lane kernels, [slots][64]
static std::vector<uint32_t> wave_slot_table(const gik_template_desc *d, const SlotLists &ents, int slots) {
  std::vector<uint32_t> meta((size_t)slots * WAVE, 0);
  for (int lane = 0; lane < WAVE; ++lane) {
    const bool active = lane < d->N * d->k;
    const int node = active ? lane / d->k : 0;
    const int comp = active ? lane % d->k : 0;
    for (int s = 0; s < slots; ++s) {
      // padding slot: this lane's own row (idle lanes: the all-zero dump row), kind none
      uint32_t m = meta_pack(active ? node : TILE_ROWS - 1, 0, 0, 0);
      if (active && s < (int)ents[node].size()) {
        const Ent &e = ents[node][s];
        m = meta_pack(e.j, e.term, e.kind, (comp == 0 && e.owner) ? 1 : 0);
      }
      meta[(size_t)s * WAVE + lane] = m;
    }
  }
  return meta;
}

// A rigid clique -- a set of nodes every pair of which is tied by an equality term (the
// anchors of a scene with many obstacles) -- is taken out of the slot tables and handled in
// closed form (gik_block.hip.h).  Greedy by equality degree; rows 0..n_clq-1 of the LDS
// arrays are the clique's nodes in ascending order, the other nodes follow.
struct CliqueRows {
  int n_clq = 0;
  std::vector<int> eqterm;        // [N][N] the equality term that ties two nodes, -1 = none
  std::vector<char> in_clq;       // [N]
  std::vector<int> node_of_row;   // [rowcap] -1 = none
  std::vector<int> nc_term;       // the terms kept in the slot tables, in the caller's order
  SlotLists ents;                 // [rowcap] their slot entries in row numbering; `term` = index in nc_term
};
static CliqueRows clique_rows(const gik_template_desc *d, int dbg, int rowcap) {
  const int N = d->N, T = d->n_terms;
  CliqueRows c;
  std::vector<int> deg(N, 0), order(N), row_of(N);
  c.eqterm.assign((size_t)N * N, -1);
  c.in_clq.assign(N, 0);
  c.node_of_row.assign(rowcap, -1);
  for (int t = 0; t < T; ++t) {
    const int i = d->term_i[t], j = d->term_j[t];
    if (d->term_kind[t] == GIK_TERM_EQ && c.eqterm[(size_t)i * N + j] < 0) {
      c.eqterm[(size_t)i * N + j] = c.eqterm[(size_t)j * N + i] = t;
      ++deg[i];
      ++deg[j];
    }
  }
  const int clique_min = (dbg & 64) ? 4 : 16;
  if (d->k == 3 && !(dbg & 128) && d->clique_closed_form != GIK_CLIQUE_OFF) {
    for (int i = 0; i < N; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return deg[a] > deg[b]; });
    std::vector<int> A;
    for (int v : order) {
      bool all = true;
      for (int a : A) all = all && c.eqterm[(size_t)v * N + a] >= 0;
      if (all) A.push_back(v);
    }
    if ((int)A.size() >= clique_min) {
      c.n_clq = (int)A.size();
      for (int a : A) c.in_clq[a] = 1;
    }
  }
  // with a clique the other nodes take the LAST rows (128 - F ...): their threads, the only
  // ones with more than a slot or two, then sit in wavefronts that have no clique work
  int r = 0;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1 && c.n_clq) r = rowcap - (N - c.n_clq);
    for (int i = 0; i < N; ++i)
      if ((c.in_clq[i] != 0) == (pass == 0)) {
        row_of[i] = r;
        c.node_of_row[r++] = i;
      }
  }
  // slot entries in row numbering, clique pairs left out; `term` = index in the LDS target table
  c.ents.assign(rowcap, {});
  for (int t = 0; t < T; ++t) {
    const int i = d->term_i[t], j = d->term_j[t], kind = d->term_kind[t];
    if (c.n_clq && kind == GIK_TERM_EQ && c.in_clq[i] && c.in_clq[j] && c.eqterm[(size_t)i * N + j] == t) continue;
    const int ri = row_of[i], rj = row_of[j], tc = (int)c.nc_term.size();
    c.nc_term.push_back(t);
    c.ents[ri].push_back({rj, kind, tc, ri < rj ? 1 : 0});
    c.ents[rj].push_back({ri, kind, tc, rj < ri ? 1 : 0});
  }
  sort_slot_lists(c.ents);
  return c;
}

// tables of the 512-thread workgroup kernels (128 rows); graphs beyond 128 nodes have none (all-zero loop bounds, one slot word)
struct BlockHost {
  std::vector<int> clq_term, clq_pair_term, wave_sl = std::vector<int>(2 * BLOCK_WAVES, 0);
  std::vector<unsigned short> clq_pid;   // [M][512] compact pair id per (thread, partner), 0xffff = none
  std::vector<uint32_t> meta = std::vector<uint32_t>(1, 0u);
  int SL = 0;      // slots per thread
};
static BlockHost block_tables(int N, int T, const CliqueRows &c) {
  BlockHost b;
  const int n_clq = c.n_clq, M = (n_clq + 3) / 4;
  b.clq_term.assign((size_t)std::max(M, 1) * BLOCK_NT, -1);
  for (int tid = 0; tid < BLOCK_NT; ++tid) {
    const int row = tid >> 2, part = tid & 3;
    for (int m = 0; m < M && row < n_clq; ++m) {
      const int j = 4 * m + part;
      if (j < n_clq && j != row)
        b.clq_term[(size_t)m * BLOCK_NT + tid] = c.eqterm[(size_t)c.node_of_row[row] * N + c.node_of_row[j]];
    }
  }
  // each clique pair once (its target is staged in LDS per problem) + the pair id of every
  // (thread, partner): ids fit 16 bits (at most 128 * 127 / 2 pairs)
  std::vector<int> pid_of_term((size_t)T, -1);
  b.clq_pid.assign((size_t)std::max(M, 1) * BLOCK_NT, (unsigned short)0xffff);
  for (size_t q = 0; q < b.clq_term.size(); ++q) {
    const int term = b.clq_term[q];
    if (term < 0) continue;
    if (pid_of_term[term] < 0) {
      pid_of_term[term] = (int)b.clq_pair_term.size();
      b.clq_pair_term.push_back(term);
    }
    b.clq_pid[q] = (unsigned short)pid_of_term[term];
  }
  // four threads per node; a node's equality terms are dealt to them in turn, then its hinge
  // terms continuing the rotation, so that both kinds spread evenly (the padded slot count of a
  // wavefront is the largest equality count plus the largest hinge count among its threads:
  // 3 + 2 -> 2 + 1 for the free nodes of the table scene).  Within a thread the equality terms
  // come first (slots [0, SLE_w): no kind decoding in the kernels) and the hinge terms last
  // (slots [SLE_w, SL_w)), with the bounds of the thread's wavefront w; unused slots are inert
  // padding (own node, kind 0, not owner)
  SlotLists eqs(BLOCK_NT), hinges(BLOCK_NT);
  for (int node = 0; node < BLOCK_MAXN; ++node) {
    int turn = 0;
    for (int pass = 0; pass < 2; ++pass)
      for (const Ent &en : c.ents[node])
        if ((en.kind == GIK_TERM_EQ) == (pass == 0))
          (pass == 0 ? eqs : hinges)[4 * node + (turn++ & 3)].push_back(en);
  }
  for (int tid = 0; tid < BLOCK_NT; ++tid) {
    const int w = tid / WAVE;
    b.wave_sl[2 * w] = std::max(b.wave_sl[2 * w], (int)eqs[tid].size());
    b.wave_sl[2 * w + 1] = std::max(b.wave_sl[2 * w + 1], (int)hinges[tid].size());
  }
  // A wavefront with few slots runs them as ONE kind-decoding loop over each thread's equality
  // terms followed by its hinge terms ({0, T_w}: T_w = most terms of any of its threads) when that
  // is shorter than the padded split loops (table scene: 1 + 1 -> 1 for the base / goal nodes,
  // 3 + 1 -> 3 for the free nodes; an iteration is two dependent LDS round trips).
  std::vector<char> merged(BLOCK_WAVES, 0);
  for (int w = 0; w < BLOCK_WAVES; ++w) {
    int tot = 0;
    for (int tid = w * WAVE; tid < (w + 1) * WAVE; ++tid)
      tot = std::max(tot, (int)(eqs[tid].size() + hinges[tid].size()));
    if (tot <= 8 && tot < b.wave_sl[2 * w] + b.wave_sl[2 * w + 1]) {
      merged[w] = 1;
      b.wave_sl[2 * w] = 0;
      b.wave_sl[2 * w + 1] = tot;
    } else {
      b.wave_sl[2 * w + 1] += b.wave_sl[2 * w];   // {SLE_w, SL_w}
    }
    b.SL = std::max(b.SL, b.wave_sl[2 * w + 1]);
  }
  b.meta.assign((size_t)std::max(b.SL, 1) * BLOCK_NT, 0);
  for (int tid = 0; tid < BLOCK_NT; ++tid) {
    const int node = tid >> 2, w = tid / WAVE, sle = merged[w] ? (int)eqs[tid].size() : b.wave_sl[2 * w];
    for (int s = 0; s < b.SL; ++s) {
      uint32_t m = meta_pack(c.node_of_row[node] >= 0 ? node : 0, 0, 0, 0);
      const std::vector<Ent> &src = s < sle ? eqs[tid] : hinges[tid];
      const int e = s < sle ? s : s - sle;
      if (e < (int)src.size()) m = meta_pack(src[e].j, src[e].term, src[e].kind, src[e].owner);
      b.meta[(size_t)s * BLOCK_NT + tid] = m;
    }
  }
  return b;
}

// ---- node-per-lane tables (gik_npt.hip.h): the host side of NptTabs, field for field ----
struct NptHost {
  bool ok = false;      // the graph fits the kernel's tables
  std::vector<int> node_of_row, clq_pair_term, term_tgt;
  std::vector<unsigned char> prow_of_slot, wslot_of_row;
  std::vector<uint32_t> term_rec;
  std::vector<unsigned short> gather;
  NptTabs n = {};       // the counts; its pointers are set by the upload, one per vector above
};
// Two layouts.  Two wavefronts per problem, one node per lane (default): the nodes outside the
// clique take the first rows, then the clique's nodes, those that carry slot terms first -- every
// end node of a slot term then sits in wavefront 0, which evaluates the terms, and the
// direction / term tables need no barrier of their own.  One wavefront, two nodes per lane
// (debug_flags 2048): the clique's nodes take rows 0..n_clq-1, the others follow; nodes that carry
// slot terms go to EVEN rows where possible, so that a lane's second node has few or none (its
// gather list is as long as the busiest second node's).
// NW wavefronts per problem ("two_waves": one node per lane, else two), `rows` thread slots
static NptHost npt_tables(const gik_template_desc *d, const CliqueRows &c, bool two_waves, int NW, int rows) {
  const int N = d->N, n_clq = c.n_clq, NSn = two_waves ? 1 : 2, NTn = NW * WAVE;
  NptHost h;
  h.n.n_clq = n_clq;
  std::vector<int> sdeg(N, 0);
  for (int t : c.nc_term) {
    ++sdeg[d->term_i[t]];
    ++sdeg[d->term_j[t]];
  }
  std::vector<int> cl_busy, cl_idle, others;
  for (int i = 0; i < N; ++i) {
    if (c.in_clq[i]) (sdeg[i] ? cl_busy : cl_idle).push_back(i);
    else others.push_back(i);
  }
  auto by_deg = [&](int a, int b) { return sdeg[a] > sdeg[b]; };
  std::stable_sort(cl_busy.begin(), cl_busy.end(), by_deg);
  std::stable_sort(others.begin(), others.end(), by_deg);
  // nrow[v]: row of node v in the point table; node_of_row[t]: node held by thread slot t
  h.node_of_row.assign(rows, -1);
  h.prow_of_slot.assign(rows, 0);
  std::vector<int> nrow(N, -1), nslot(N, -1);
  int n_rows = 0;
  if (two_waves) {
    h.n.cbase = (int)others.size();
    int r = 0;
    for (int v : others) nrow[v] = r++;
    for (int v : cl_busy) nrow[v] = r++;
    for (int v : cl_idle) nrow[v] = r++;
    n_rows = r;
    // thread slots: the nodes that carry slot terms on the even lanes 0, 2, ... of wavefront 0, each with a
    // clique node WITHOUT slot terms next to it (its helper in the gather); everything else behind
    std::vector<int> busy(others.begin(), others.end());
    busy.insert(busy.end(), cl_busy.begin(), cl_busy.end());
    busy.erase(std::remove_if(busy.begin(), busy.end(), [&](int v) { return sdeg[v] == 0; }), busy.end());
    std::stable_sort(busy.begin(), busy.end(), by_deg);
    std::vector<char> placed(N, 0);
    int slot = 0;
    size_t ih = 0;
    const bool can_help = 2 * busy.size() <= (size_t)WAVE && cl_idle.size() >= busy.size();
    for (int v : busy) {
      h.node_of_row[slot] = v;
      nslot[v] = slot++;
      placed[v] = 1;
      if (can_help) {
        const int hn = cl_idle[ih++];
        h.node_of_row[slot] = hn;
        nslot[hn] = slot++;
        placed[hn] = 1;
      }
    }
    h.n.n_helped = can_help ? (int)busy.size() : 0;
    for (int pass = 0; pass < 3; ++pass)
      for (int v : (pass == 0 ? others : (pass == 1 ? cl_busy : cl_idle)))
        if (!placed[v]) {
          h.node_of_row[slot] = v;
          nslot[v] = slot++;
          placed[v] = 1;
        }
  } else {
    h.n.cbase = 0;
    size_t ib = 0, ii = 0;
    for (int r = 0; r < n_clq; ++r) {
      const bool want_busy = (r & 1) == 0;
      int v;
      if ((want_busy && ib < cl_busy.size()) || ii >= cl_idle.size()) v = cl_busy[ib++];
      else v = cl_idle[ii++];
      nrow[v] = r;
    }
    const int start = (n_clq + 1) & ~1;
    const bool even_only = others.empty() || start + 2 * ((int)others.size() - 1) < rows;
    n_rows = n_clq;
    for (size_t q = 0; q < others.size(); ++q) {
      const int r = even_only ? start + 2 * (int)q : n_clq + (int)q;
      nrow[others[q]] = r;
      n_rows = r + 1;
    }
    for (int v = 0; v < N; ++v) {      // thread slot = row
      h.node_of_row[nrow[v]] = v;
      nslot[v] = nrow[v];
    }
  }
  for (int v = 0; v < N; ++v) h.prow_of_slot[nslot[v]] = (unsigned char)nrow[v];
  h.n.n_rows = (n_rows + 1) & ~1;
  // compact direction table: one row per node that carries slot terms
  h.wslot_of_row.assign(rows, 255);
  int n_wrows = 0;
  std::vector<int> wslot_of_node(N, 255);
  for (int t = 0; t < rows; ++t)
    if (h.node_of_row[t] >= 0 && sdeg[h.node_of_row[t]]) {
      wslot_of_node[h.node_of_row[t]] = n_wrows;
      h.wslot_of_row[t] = (unsigned char)n_wrows++;
      if (two_waves && t >= WAVE) h.n.term_sync = 1;
    }
  const int Tn = (int)c.nc_term.size();
  if (Tn > 64 * 4 || n_wrows > 127) return h;
  h.n.TL = Tn <= 64 ? 1 : 4;
  h.term_rec.assign((size_t)h.n.TL * WAVE, 0u);
  h.term_tgt.assign((size_t)h.n.TL * WAVE, -1);
  for (size_t q = 0; q < h.term_rec.size(); ++q)   // padding: rows 0 / 0, kind 0, the zero direction row
    h.term_rec[q] = ((uint32_t)n_wrows << 18) | ((uint32_t)n_wrows << 25);
  struct GEnt { int other, kind, slot, neg; };
  std::vector<std::vector<GEnt>> glist(rows);
  for (int q = 0; q < Tn; ++q) {
    const int t = c.nc_term[q], i = d->term_i[t], j = d->term_j[t], kind = d->term_kind[t];
    const int ri = nrow[i], rj = nrow[j];
    h.term_rec[q] = (uint32_t)ri | ((uint32_t)rj << 8) | ((uint32_t)kind << 16) |
                    ((uint32_t)wslot_of_node[i] << 18) | ((uint32_t)wslot_of_node[j] << 25);
    h.term_tgt[q] = t;
    // term slot q = u * 64 + lane: the order of nc_term (= the reference's edge order)
    glist[nslot[i]].push_back({j, kind, q, 0});
    glist[nslot[j]].push_back({i, kind, q, 1});
  }
  int deg[2] = {0, 0};
  for (int r = 0; r < rows; ++r)
    std::stable_sort(glist[r].begin(), glist[r].end(), [](const GEnt &a, const GEnt &b) {
      return a.other != b.other ? a.other < b.other : a.kind < b.kind;
    });
  for (int i = 0; i < h.n.n_helped; ++i) {      // the second half of a busy node's list moves to its helper
    std::vector<GEnt> &own = glist[2 * i], &hlp = glist[2 * i + 1];
    const size_t keep = (own.size() + 1) / 2;
    hlp.assign(own.begin() + keep, own.end());
    own.resize(keep);
  }
  for (int r = 0; r < rows; ++r) {
    const int sl = NSn == 1 ? 0 : (r & 1);
    deg[sl] = std::max(deg[sl], (int)glist[r].size());
  }
  h.n.DEG0 = deg[0];
  h.n.DEG1 = deg[1];
  const unsigned short pad = (unsigned short)(2 * Tn);
  h.gather.assign((size_t)std::max(1, deg[0] + deg[1]) * NTn, pad);
  for (int r = 0; r < rows; ++r) {
    const int thr = r / NSn, sl = r % NSn;
    for (size_t e = 0; e < glist[r].size(); ++e)
      h.gather[(size_t)(sl ? deg[0] + (int)e : (int)e) * NTn + thr] =
          (unsigned short)((glist[r][e].slot << 1) | glist[r][e].neg);
  }
  std::vector<int> node_at_row(rows, 0);
  for (int v = 0; v < N; ++v) node_at_row[nrow[v]] = v;
  for (int a = 0; a < c.n_clq; ++a)
    for (int b = a + 1; b < c.n_clq; ++b)
      h.clq_pair_term.push_back(c.eqterm[(size_t)node_at_row[h.n.cbase + a] * N + node_at_row[h.n.cbase + b]]);
  h.n.n_pairs = (int)h.clq_pair_term.size();
  h.n.n_wrows = n_wrows;
  h.n.n_terms = Tn;
  h.ok = deg[0] + deg[1] <= 16;      // NptCtx::NG packed words
  return h;
}

// The tables of seed_kernel: T0[parent]^-1 T0[j] per joint, the parents along the end-effector paths, a root-first
// order, and per graph node where graph.realization puts it (_pose_goal, graph_revolute.py:243-249: p_j = trans F_j,
// q_j = p_j + axis_length z_j; graph_planar.py:136-145: every child u pins p_u = trans F_u and its parent
// p_parent = p_u - |parent u| x_u, the last child in get_all_poses' order winning; nodes it does not name keep
// their POS: anchor_pos).  A graph the recipe does not cover has ok false, and `why` says why.
struct SeedRecipe {
  std::vector<double> Trel, coef;            // [n + 1][(K + 1)^2], [N]
  std::vector<int> parent, order, frame, anchor;   // parent: as uploaded, -1 = a root or a joint on no path
  bool ok = false;
  std::string why;
};
static SeedRecipe seed_recipe(int N, int K, const gik_pipeline_desc *d, const std::vector<int> &path, int n_ee) {
  const int D = K + 1, DD = D * D, n = d->n_joints;
  SeedRecipe s;
  std::vector<int> parent(n + 1, -2), order;
  for (int e = 0; e < n_ee; ++e)
    for (int k = 0; k <= n; ++k) {
      const int j = path[(size_t)e * (n + 1) + k];
      if (j < 0) break;
      const int p = k == 0 ? -1 : path[(size_t)e * (n + 1) + k - 1];
      if (parent[j] == -2) {
        parent[j] = p;
        order.push_back(j);
      } else if (parent[j] != p) {
        s.why = "joint " + std::to_string(j) + " has two parents on the end-effector paths";
        return s;
      }
    }
  std::vector<double> Trel((size_t)(n + 1) * DD, 0.0);
  for (int j : order) {
    const int p = parent[j];
    if (p < 0) continue;
    const double *A = d->T0 + (size_t)p * DD, *B = d->T0 + (size_t)j * DD;
    double *R = Trel.data() + (size_t)j * DD;
    // rigid inverse of A times B: rotation A_R^T B_R, translation A_R^T (B_t - A_t)
    for (int r = 0; r < K; ++r) {
      for (int c = 0; c < K; ++c) {
        double acc = 0.0;
        for (int u = 0; u < K; ++u) acc += A[u * D + r] * B[u * D + c];
        R[r * D + c] = acc;
      }
      double acc = 0.0;
      for (int u = 0; u < K; ++u) acc += A[u * D + r] * (B[u * D + K] - A[u * D + K]);
      R[r * D + K] = acc;
    }
    R[K * D + K] = 1.0;
  }
  std::vector<int> frame(N, -1), anchor(N, -1);
  std::vector<double> coef(N, 0.0);
  for (int a = 0; a < d->n_anchor; ++a)
    if (d->anchor_index[a] >= 0 && d->anchor_index[a] < N) anchor[d->anchor_index[a]] = a;
  for (int j : order) {
    if (K == 3) {
      frame[d->p_index[j]] = j;
      coef[d->p_index[j]] = 0.0;
      frame[d->q_index[j]] = j;
      coef[d->q_index[j]] = d->axis_length;
    } else if (parent[j] >= 0) {
      const double *R = Trel.data() + (size_t)j * DD;
      frame[d->p_index[j]] = j;
      coef[d->p_index[j]] = 0.0;
      frame[d->p_index[parent[j]]] = j;
      coef[d->p_index[parent[j]]] = -std::sqrt(R[0 * D + K] * R[0 * D + K] + R[1 * D + K] * R[1 * D + K]);
    }
  }
  for (int i = 0; i < N; ++i)
    if (frame[i] < 0 && anchor[i] < 0) {
      s.why = "graph node " + std::to_string(i) + " is placed by neither a joint frame nor an anchor";
      return s;
    }
  for (int &p : parent) p = p < -1 ? -1 : p;
  s.Trel = Trel;
  s.parent = parent;
  s.order = order;
  s.frame = frame;
  s.coef = coef;
  s.anchor = anchor;
  s.ok = true;
  return s;
}

// hinges = 1: the per-node link records of WaveCtx<.., LINKS> ([ANCH_LMAX][ANCH_LROWS], zero = no link), or the reason of a
// refusal (empty = fine).  A link end is a free node or a row of the anchor table; a link with two constant ends carries no
// hinge (it is still measured).  maxdeg, slot_meta, free_full, anchor_full: the template's slot count, its slot table and
// the rows of its free nodes and of its anchors in the full point matrix
static std::string link_hinge_records(int N, int maxdeg, const std::vector<uint32_t> &slot_meta, const std::vector<int> &free_full,
                                      const std::vector<int> &anchor_full, const gik_link_desc *d, std::vector<AnchLinkRec> &recs) {
  if (maxdeg != 9)
    return "hinges = 1 needs the 9-slot fixed-anchor kernel; this template runs the " + std::to_string(maxdeg) +
           "-slot variant, which has no link hinges";
  recs.assign((size_t)ANCH_LMAX * ANCH_LROWS, AnchLinkRec{0.0, 0u, 0u});
  std::vector<int> cnt(N, 0);
  // full row -> free node, or anchor row, or neither
  auto find = [](const std::vector<int> &v, int row) {
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i] == row) return (int)i;
    return -1;
  };
  // the slot of free node i whose neighbour is free node j (a real term, not padding), or -1
  auto slot_to = [&](int i, int j) {
    for (int s = 0; s < maxdeg; ++s) {
      const uint32_t m = slot_meta[(size_t)s * WAVE + i * 3];
      if (((m >> 24) & 3u) != 0u && meta_j(m) == j) return s;
    }
    return -1;
  };
  for (int l = 0; l < d->n_link; ++l) {
    const int row[2] = {d->link_a[l], d->link_b[l]};
    int fr[2], an[2];
    for (int q = 0; q < 2; ++q) {
      fr[q] = find(free_full, row[q]);
      an[q] = fr[q] < 0 ? find(anchor_full, row[q]) : -1;
      if (fr[q] < 0 && an[q] < 0)
        return "hinges = 1: link " + std::to_string(l) + " ends at row " + std::to_string(row[q]) +
               ", which is neither a free node nor an anchor row";
    }
    if (fr[0] < 0 && fr[1] < 0) continue;
    int slot[2] = {0xff, 0xff};
    if (fr[0] >= 0 && fr[1] >= 0) {
      slot[0] = slot_to(fr[0], fr[1]);
      slot[1] = slot_to(fr[1], fr[0]);
      if (fr[0] == fr[1] || slot[0] < 0 || slot[1] < 0)
        return "hinges = 1: the two free ends of link " + std::to_string(l) + " share no term";
    }
    for (int q = 0; q < 2; ++q) {
      if (fr[q] < 0) continue;
      if (cnt[fr[q]] >= ANCH_LMAX)
        return "hinges = 1: more than " + std::to_string(ANCH_LMAX) + " hinge links at free node " + std::to_string(fr[q]);
      const bool oc = fr[1 - q] < 0;
      AnchLinkRec &r = recs[(size_t)cnt[fr[q]]++ * ANCH_LROWS + fr[q]];
      r.rho = d->link_radius[l];
      r.meta = link_meta_pack(q, oc ? 1 : 0, oc ? an[1 - q] : fr[1 - q], slot[q]);
    }
  }
  return "";
}

// The descriptors of WaveCtx<.., SELF> ([ANCH_SELF_HMAX], zero = unused), or the reason of a refusal: pair p's four ends
// a_l, b_l, a_m, b_m as offsets from the tiles (a free row: 6 * row; an anchor row: 0x8000 | 4 * row) and R = rho_l + rho_m.
static std::string self_hinge_descs(const std::vector<int> &free_full, const std::vector<int> &anchor_full, const std::vector<int> &link_a,
                                    const std::vector<int> &link_b, const std::vector<double> &link_rho, const std::vector<int> &pair_l,
                                    const std::vector<int> &pair_m, std::vector<AnchSelfDesc> &descs) {
  descs.assign((size_t)ANCH_SELF_HMAX, AnchSelfDesc{{0, 0, 0, 0}, 0.0});
  auto find = [](const std::vector<int> &v, int row) {
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i] == row) return (int)i;
    return -1;
  };
  for (size_t p = 0; p < pair_l.size(); ++p) {
    const int link[2] = {pair_l[p], pair_m[p]};
    for (int q = 0; q < 4; ++q) {
      const int l = link[q >> 1], row = (q & 1) ? link_b[l] : link_a[l];
      const int fr = find(free_full, row), an = fr < 0 ? find(anchor_full, row) : -1;
      if (fr < 0 && an < 0)
        return "link " + std::to_string(l) + " of pair " + std::to_string(p) + " ends at row " + std::to_string(row) +
               ", which is neither a free node nor an anchor row";
      descs[p].off[q] = (uint16_t)(fr >= 0 ? 6 * fr : (0x8000 | (4 * an)));
    }
    descs[p].R = link_rho[link[0]] + link_rho[link[1]];
  }
  return "";
}

}  // namespace gik
