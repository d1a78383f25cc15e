// tests/host/tables_walk.cpp -- the host tables of a template (graphik_amd/csrc/gik_tables.hip.h) built on the CPU, as a
// program of its own: for every case of the files named on the command line it runs the builders in the order
// create_impl, gik_pipeline_attach and gik_anchored_attach_links chain them, asserts what makes a table safe to hand to a
// kernel (every packed row, term, slot and pair id inside its table), and prints per table its length and a 64-bit
// FNV-1a of its bytes, next to the scalar fields and the reasons of refusals, as JSON.  tests/test_host_tables.py writes
// the case files, compiles this (host only, address and undefined-behaviour sanitizers) and compares the output with
// tests/golden/host_tables.json (docs/NOTEBOOK.md 28).
//
// Case files are blank-separated tokens; doubles in C's hexadecimal notation.
//   tables NAME N k T clique_closed_form dbg two_waves NW rows n_slots slots.. term_i[T] term_j[T] term_kind[T]
//   seed   NAME N K n_joints n_anchor n_ee axis_length T0[(n+1)(K+1)^2] p_index[n+1] q_index[n+1] anchor_index[n_anchor]
//          path[n_ee (n+1)]
//   links  NAME N T slots term_i[T] term_j[T] term_kind[T] free_full[N] n_anchor anchor_full[n_anchor] n_link link_a[]
//          link_b[] link_radius[]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "gik_tables.hip.h"

using namespace gik;

// ---- input -----------------------------------------------------------------------------------------------------
struct Reader {
  FILE *f;
  bool word(std::string &s) {
    char buf[256];
    if (std::fscanf(f, "%255s", buf) != 1) return false;
    s = buf;
    return true;
  }
  std::string word() {
    std::string s;
    if (!word(s)) {
      std::fprintf(stderr, "case file ends inside a case\n");
      std::exit(2);
    }
    return s;
  }
  int i() { return (int)std::strtol(word().c_str(), nullptr, 10); }
  double d() { return std::strtod(word().c_str(), nullptr); }
  std::vector<int> ints(int n) {
    std::vector<int> v((size_t)std::max(n, 0));
    for (int &x : v) x = i();
    return v;
  }
  std::vector<double> doubles(int n) {
    std::vector<double> v((size_t)std::max(n, 0));
    for (double &x : v) x = d();
    return v;
  }
};

// ---- output ----------------------------------------------------------------------------------------------------
static int g_broken = 0;
static std::string g_case;
#define CHECK(c)                                                                                  \
  do {                                                                                            \
    if (!(c)) {                                                                                   \
      if (++g_broken <= 40) std::fprintf(stderr, "BROKEN %s: line %d: %s\n", g_case.c_str(), __LINE__, #c); \
    }                                                                                             \
  } while (0)

static const char *g_sep = "";
static void field(const char *name) {
  std::printf("%s\"%s\": ", g_sep, name);
  g_sep = ", ";
}
static void num(const char *name, long long v) {
  field(name);
  std::printf("%lld", v);
}
static void str(const char *name, const std::string &s) {
  field(name);
  std::printf("\"%s\"", s.c_str());      // (the reasons hold neither quotes nor backslashes)
}
template <typename T>
static void tab(const char *name, const std::vector<T> &v) {
  uint64_t h = 0xcbf29ce484222325ull;
  const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
  for (size_t q = 0; q < v.size() * sizeof(T); ++q) h = (h ^ p[q]) * 0x100000001b3ull;
  field(name);
  std::printf("[%zu, \"%016llx\"]", v.size(), (unsigned long long)h);
}
static void list(const char *name, const std::vector<int> &v) {
  field(name);
  std::printf("[");
  for (size_t q = 0; q < v.size(); ++q) std::printf("%s%d", q ? ", " : "", v[q]);
  std::printf("]");
}
static std::vector<int> flat(const SlotLists &l) {
  std::vector<int> v;
  for (const auto &e : l) {
    v.push_back((int)e.size());
    for (const Ent &x : e) v.insert(v.end(), {x.j, x.kind, x.term, x.owner});
  }
  return v;
}

static int w_term(uint32_t m) { return (int)((m >> 8) & 0xffffu); }
static int w_kind(uint32_t m) { return (int)((m >> 24) & 3u); }
static int w_owner(uint32_t m) { return (int)((m >> 26) & 1u); }

// every term of [0, n_terms) sits in exactly two of the lists, in one of them as owner
static void check_lists(const SlotLists &l, int rows_max, int n_terms) {
  std::vector<int> seen((size_t)n_terms, 0), own((size_t)n_terms, 0);
  for (size_t r = 0; r < l.size(); ++r)
    for (const Ent &e : l[r]) {
      CHECK(e.j >= 0 && e.j < rows_max && e.j != (int)r && e.term >= 0 && e.term < n_terms);
      CHECK(e.kind >= GIK_TERM_EQ && e.kind <= GIK_TERM_UPPER);
      if (e.term >= 0 && e.term < n_terms) {
        ++seen[e.term];
        own[e.term] += e.owner;
      }
    }
  for (int t = 0; t < n_terms; ++t) CHECK(seen[t] == 2 && own[t] == 1);
}

// ---- the creation tables ---------------------------------------------------------------------------------------
static void wave_case(const gik_template_desc &d, const SlotLists &ents, int slots) {
  const std::vector<uint32_t> meta = wave_slot_table(&d, ents, slots);
  char name[32];
  std::snprintf(name, sizeof name, "wave%d", slots);
  tab(name, meta);
  CHECK((int)meta.size() == slots * WAVE);
  std::vector<int> seen((size_t)d.n_terms, 0), own((size_t)d.n_terms, 0);
  for (int s = 0; s < slots; ++s)
    for (int lane = 0; lane < WAVE; ++lane) {
      const uint32_t m = meta[(size_t)s * WAVE + lane];
      const bool active = lane < d.N * d.k;
      CHECK(meta_j(m) < TILE_ROWS);
      if (w_kind(m) == 0) {      // padding: the lane's own row or the dump row
        CHECK(meta_j(m) == (active ? lane / d.k : TILE_ROWS - 1) && w_term(m) == 0 && w_owner(m) == 0);
        continue;
      }
      CHECK(active && meta_j(m) < d.N && meta_j(m) != lane / d.k && w_term(m) < d.n_terms);
      CHECK(lane % d.k == 0 || w_owner(m) == 0);
      if (active && lane % d.k == 0 && w_term(m) < d.n_terms) {
        ++seen[w_term(m)];
        own[w_term(m)] += w_owner(m);
      }
    }
  for (int t = 0; t < d.n_terms; ++t) CHECK(seen[t] == 2 && own[t] == 1);
}

static void block_case(const gik_template_desc &d, const CliqueRows &c) {
  const BlockHost b = block_tables(d.N, d.n_terms, c);
  const int Tc = (int)c.nc_term.size(), n_pairs = (int)b.clq_pair_term.size();
  tab("clq_term", b.clq_term);
  tab("clq_pair_term", b.clq_pair_term);
  tab("clq_pid", b.clq_pid);
  tab("block_meta", b.meta);
  list("wave_sl", b.wave_sl);
  num("SL", b.SL);
  CHECK((int)b.wave_sl.size() == 2 * BLOCK_WAVES && (int)b.meta.size() == std::max(b.SL, 1) * BLOCK_NT);
  for (int w = 0; w < BLOCK_WAVES; ++w) CHECK(0 <= b.wave_sl[2 * w] && b.wave_sl[2 * w] <= b.wave_sl[2 * w + 1] && b.wave_sl[2 * w + 1] <= b.SL);
  // the slot words
  std::vector<int> seen((size_t)Tc, 0), own((size_t)Tc, 0), eq_in_wave(BLOCK_WAVES, 0), terms_in_wave(BLOCK_WAVES, 0);
  for (int s = 0; s < b.SL; ++s)
    for (int tid = 0; tid < BLOCK_NT; ++tid) {
      const uint32_t m = b.meta[(size_t)s * BLOCK_NT + tid];
      const int node = tid >> 2, w = tid / WAVE;
      CHECK(meta_j(m) < BLOCK_MAXN);
      if (w_kind(m) == 0) {
        CHECK(meta_j(m) == (c.node_of_row[node] >= 0 ? node : 0) && w_term(m) == 0 && w_owner(m) == 0);
        continue;
      }
      CHECK(s < b.wave_sl[2 * w + 1] && c.node_of_row[node] >= 0 && c.node_of_row[meta_j(m)] >= 0 && w_term(m) < Tc);
      // below the wavefront's first bound only equalities, no kind decoding there
      CHECK(s >= b.wave_sl[2 * w] || w_kind(m) == GIK_TERM_EQ);
      ++terms_in_wave[w];
      eq_in_wave[w] += w_kind(m) == GIK_TERM_EQ;
      if (w_term(m) < Tc) {
        ++seen[w_term(m)];
        own[w_term(m)] += w_owner(m);
      }
    }
  for (int t = 0; t < Tc; ++t) CHECK(seen[t] == 2 && own[t] == 1);
  int merged = 0, split = 0;      // a wavefront that runs its equalities inside the kind-decoding loop / in a loop of their own
  for (int w = 0; w < BLOCK_WAVES; ++w) {
    merged += eq_in_wave[w] > 0 && b.wave_sl[2 * w] == 0;
    split += eq_in_wave[w] > 0 && eq_in_wave[w] < terms_in_wave[w] && b.wave_sl[2 * w] > 0;
  }
  num("merged_waves", merged);
  num("split_waves", split);
  // the clique's pairs
  CHECK(n_pairs == c.n_clq * (c.n_clq - 1) / 2);
  CHECK(b.clq_pid.size() == b.clq_term.size());
  for (size_t q = 0; q < b.clq_pid.size(); ++q) {
    CHECK(b.clq_pid[q] == 0xffff || b.clq_pid[q] < n_pairs);
    CHECK((b.clq_pid[q] == 0xffff) == (b.clq_term[q] < 0));
    if (b.clq_pid[q] != 0xffff && b.clq_pid[q] < n_pairs) CHECK(b.clq_pair_term[b.clq_pid[q]] == b.clq_term[q]);
  }
  std::set<int> once;
  for (int t : b.clq_pair_term) {
    CHECK(t >= 0 && t < d.n_terms && once.insert(t).second);
    if (t >= 0 && t < d.n_terms) CHECK(d.term_kind[t] == GIK_TERM_EQ && c.in_clq[d.term_i[t]] && c.in_clq[d.term_j[t]]);
  }
}

static void npt_case(const gik_template_desc &d, const CliqueRows &c, bool two_waves, int NW, int rows) {
  const NptHost h = npt_tables(&d, c, two_waves, NW, rows);
  const NptTabs &n = h.n;
  num("npt_ok", h.ok);
  num("npt_NW", NW);
  tab("npt_node_of_row", h.node_of_row);
  tab("npt_prow_of_slot", h.prow_of_slot);
  tab("npt_wslot_of_row", h.wslot_of_row);
  tab("npt_clq_pair_term", h.clq_pair_term);
  tab("npt_term_rec", h.term_rec);
  tab("npt_term_tgt", h.term_tgt);
  tab("npt_gather", h.gather);
  list("npt_counts", {n.n_clq, n.n_pairs, n.DEG0, n.DEG1, n.n_wrows, n.TL, n.clq_euclid, n.cbase, n.n_rows, n.n_terms, n.term_sync,
                      n.n_helped});
  if (!h.ok) return;
  const int Tn = n.n_terms;
  CHECK(Tn == (int)c.nc_term.size() && n.n_rows <= rows && n.n_wrows <= 127 && n.DEG0 + n.DEG1 <= 16);
  CHECK(n.n_clq == c.n_clq && n.n_pairs == n.n_clq * (n.n_clq - 1) / 2 && (int)h.clq_pair_term.size() == n.n_pairs);
  CHECK((n.TL == 1 || n.TL == 4) && Tn <= n.TL * WAVE && (int)h.term_rec.size() == n.TL * WAVE && h.term_tgt.size() == h.term_rec.size());
  // the nodes onto the rows of the point table, one to one
  std::set<int> nodes, prows;
  CHECK((int)h.node_of_row.size() == rows && (int)h.prow_of_slot.size() == rows && (int)h.wslot_of_row.size() == rows);
  for (int s = 0; s < rows; ++s) {
    if (h.node_of_row[s] < 0) continue;
    CHECK(h.node_of_row[s] < d.N && nodes.insert(h.node_of_row[s]).second);
    CHECK(h.prow_of_slot[s] < n.n_rows && prows.insert(h.prow_of_slot[s]).second);
    CHECK(h.wslot_of_row[s] == 255 || h.wslot_of_row[s] < n.n_wrows);
  }
  CHECK((int)nodes.size() == d.N && (int)prows.size() == d.N);
  // term records: rows of the point table, rows of the direction table, the term's own kind; padding: kind 0, the zero row
  for (int q = 0; q < (int)h.term_rec.size(); ++q) {
    const uint32_t rec = h.term_rec[q];
    const int ri = (int)(rec & 0xffu), rj = (int)((rec >> 8) & 0xffu), kind = (int)((rec >> 16) & 3u);
    const int wi = (int)((rec >> 18) & 0x7fu), wj = (int)((rec >> 25) & 0x7fu);
    CHECK(ri < n.n_rows && rj < n.n_rows && wi <= n.n_wrows && wj <= n.n_wrows);
    if (q < Tn) {
      const int t = h.term_tgt[q];
      CHECK(t >= 0 && t < d.n_terms && t == c.nc_term[q] && ri != rj && wi < n.n_wrows && wj < n.n_wrows);
      if (t >= 0 && t < d.n_terms) CHECK(kind == d.term_kind[t] && kind >= GIK_TERM_EQ && kind <= GIK_TERM_UPPER);
    } else {
      CHECK(kind == 0 && h.term_tgt[q] == -1 && wi == n.n_wrows && wj == n.n_wrows);
    }
  }
  // gather lists: every term slot once with each sign
  CHECK((int)h.gather.size() == std::max(1, n.DEG0 + n.DEG1) * NW * WAVE);
  std::vector<int> hits((size_t)2 * Tn, 0);
  for (unsigned short g : h.gather) {
    CHECK(g == 2 * Tn || (g >> 1) < Tn);
    if (g < 2 * Tn) ++hits[g];
  }
  for (int q = 0; q < 2 * Tn; ++q) CHECK(hits[q] == 1);
  for (int t : h.clq_pair_term) CHECK(t >= 0 && t < d.n_terms && d.term_kind[t] == GIK_TERM_EQ);
}

static void tables_case(Reader &in) {
  gik_template_desc d = {};
  d.N = in.i();
  d.k = in.i();
  d.n_terms = in.i();
  d.clique_closed_form = in.i();
  const int dbg = in.i(), two_waves = in.i(), NW = in.i(), rows = in.i();
  const std::vector<int> slots = in.ints(in.i());
  const std::vector<int> ti = in.ints(d.n_terms), tj = in.ints(d.n_terms), tk = in.ints(d.n_terms);
  d.term_i = ti.data();
  d.term_j = tj.data();
  d.term_kind = tk.data();
  d.debug_flags = dbg;
  num("N", d.N);
  num("k", d.k);
  num("T", d.n_terms);
  if (d.N < 2 || d.N > 255) {      // (validate_desc: no table is built)
    str("refused", "N");
    return;
  }
  SlotLists ents;
  int maxdeg = -1;
  const std::string why = slot_lists(&d, ents, maxdeg);
  str("slot_lists", why);
  if (!why.empty()) return;
  num("maxdeg", maxdeg);
  tab("ents", flat(ents));
  CHECK((int)ents.size() == d.N);
  check_lists(ents, d.N, d.n_terms);
  // one unknown per lane: every compiled slot count that holds the busiest node
  if (d.N * d.k <= WAVE && d.N <= 32)
    for (int s : slots)
      if (s >= maxdeg) wave_case(d, ents, s);
  // a workgroup per problem, and the node-per-lane kernel next to it
  const bool big = d.N > BLOCK_MAXN;
  const int rowcap = big ? 256 : BLOCK_MAXN;
  const CliqueRows c = clique_rows(&d, dbg, rowcap);
  num("n_clq", c.n_clq);
  tab("eqterm", c.eqterm);
  tab("in_clq", c.in_clq);
  tab("node_of_row", c.node_of_row);
  tab("nc_term", c.nc_term);
  tab("clq_ents", flat(c.ents));
  CHECK((int)c.node_of_row.size() == rowcap && (int)c.ents.size() == rowcap);
  std::set<int> placed;
  for (int r = 0; r < rowcap; ++r)
    if (c.node_of_row[r] >= 0) CHECK(c.node_of_row[r] < d.N && placed.insert(c.node_of_row[r]).second && (r < c.n_clq) == (c.in_clq[c.node_of_row[r]] != 0));
  CHECK((int)placed.size() == d.N);
  check_lists(c.ents, rowcap, (int)c.nc_term.size());
  if (!big) block_case(d, c);
  if (d.k == 3) {
    if (rows < d.N || rows > 256 || NW < 1 || NW * WAVE * (two_waves ? 1 : 2) < rows) {
      std::fprintf(stderr, "%s: bad layout arguments\n", g_case.c_str());
      std::exit(2);
    }
    npt_case(d, c, two_waves != 0, NW, rows);
  }
}

// ---- the FK recipe of seed_kernel ------------------------------------------------------------------------------
static void seed_case(Reader &in) {
  gik_pipeline_desc d = {};
  const int N = in.i(), K = in.i();
  d.n_joints = in.i();
  d.n_anchor = in.i();
  const int n_ee = in.i(), n = d.n_joints, DD = (K + 1) * (K + 1);
  d.axis_length = in.d();
  const std::vector<double> T0 = in.doubles((n + 1) * DD);
  const std::vector<int> p = in.ints(n + 1), q = in.ints(n + 1), ai = in.ints(d.n_anchor), path = in.ints(n_ee * (n + 1));
  d.T0 = T0.data();
  d.p_index = p.data();
  d.q_index = q.data();
  d.anchor_index = ai.data();
  const SeedRecipe s = seed_recipe(N, K, &d, path, n_ee);
  num("N", N);
  num("K", K);
  num("seed_ok", s.ok);
  str("seed_why", s.why);
  if (!s.ok) return;
  tab("Trel", s.Trel);
  tab("parent", s.parent);
  tab("order", s.order);
  tab("frame", s.frame);
  tab("coef", s.coef);
  tab("anchor", s.anchor);
  CHECK((int)s.Trel.size() == (n + 1) * DD && (int)s.parent.size() == n + 1 && (int)s.order.size() <= n + 1);
  CHECK((int)s.frame.size() == N && (int)s.coef.size() == N && (int)s.anchor.size() == N);
  // root first: a joint's parent comes before it
  std::set<int> done;
  for (int j : s.order) {
    CHECK(j >= 0 && j <= n && done.insert(j).second);
    if (j < 0 || j > n) continue;
    CHECK(s.parent[j] == -1 || done.count(s.parent[j]));
    if (s.parent[j] < 0)
      for (int e = 0; e < DD; ++e) CHECK(s.Trel[(size_t)j * DD + e] == 0.0);
  }
  for (int j = 0; j <= n; ++j) CHECK(s.parent[j] >= -1 && s.parent[j] <= n);
  for (int i = 0; i < N; ++i) {
    CHECK((s.frame[i] >= 0 && done.count(s.frame[i])) || (s.frame[i] == -1 && s.anchor[i] >= 0));
    CHECK(s.anchor[i] >= -1 && s.anchor[i] < d.n_anchor);
  }
}

// ---- the link records of the fixed-anchor solve ----------------------------------------------------------------
static void links_case(Reader &in) {
  gik_template_desc d = {};
  d.N = in.i();
  d.k = 3;
  d.n_terms = in.i();
  const int slots = in.i();
  const std::vector<int> ti = in.ints(d.n_terms), tj = in.ints(d.n_terms), tk = in.ints(d.n_terms);
  d.term_i = ti.data();
  d.term_j = tj.data();
  d.term_kind = tk.data();
  const std::vector<int> free_full = in.ints(d.N), anchor_full = in.ints(in.i());
  gik_link_desc ld = {};
  ld.n_link = in.i();
  ld.hinges = 1;
  const std::vector<int> la = in.ints(ld.n_link), lb = in.ints(ld.n_link);
  const std::vector<double> rho = in.doubles(ld.n_link);
  ld.link_a = la.data();
  ld.link_b = lb.data();
  ld.link_radius = rho.data();
  SlotLists ents;
  int maxdeg = -1;
  const std::string bad = slot_lists(&d, ents, maxdeg);
  if (!bad.empty() || d.N * 3 > WAVE || maxdeg > slots) {
    std::fprintf(stderr, "%s: not a fixed-anchor graph\n", g_case.c_str());
    std::exit(2);
  }
  const std::vector<uint32_t> meta = wave_slot_table(&d, ents, slots);
  std::vector<AnchLinkRec> recs;
  const std::string why = link_hinge_records(d.N, slots, meta, free_full, anchor_full, &ld, recs);
  num("N", d.N);
  num("slots", slots);
  num("maxdeg", maxdeg);
  str("links_why", why);
  if (!why.empty()) return;
  tab("recs", recs);
  CHECK((int)recs.size() == ANCH_LMAX * ANCH_LROWS && d.N < ANCH_LROWS);
  int n_rec = 0;
  for (int l = 0; l < ANCH_LMAX; ++l)
    for (int row = 0; row < ANCH_LROWS; ++row) {
      const AnchLinkRec &r = recs[(size_t)l * ANCH_LROWS + row];
      if (!(r.meta & 1u)) {
        CHECK(r.meta == 0u && r.rho == 0.0);
        continue;
      }
      ++n_rec;
      const int other_const = (int)((r.meta >> 2) & 1u), other = (int)((r.meta >> 8) & 0xffu), slot = (int)((r.meta >> 16) & 0xffu);
      CHECK(row < d.N && r.rho >= 0.0 && r.pad == 0u);
      CHECK(l == 0 || (recs[(size_t)(l - 1) * ANCH_LROWS + row].meta & 1u));      // a node's records are its first ones
      if (other_const) {
        CHECK(slot == 0xff && other < (int)anchor_full.size());
      } else {
        // a real term of this node whose neighbour is the other end
        CHECK(other < d.N && other != row && slot < slots);
        if (row < d.N && slot < slots) {
          const uint32_t m = meta[(size_t)slot * WAVE + row * 3];
          CHECK(w_kind(m) != 0 && meta_j(m) == other);
        }
      }
    }
  num("n_rec", n_rec);
}

int main(int argc, char **argv) {
  std::printf("{\"cases\": [");
  const char *sep = "";
  for (int a = 1; a < argc; ++a) {
    Reader in{std::fopen(argv[a], "r")};
    if (!in.f) {
      std::fprintf(stderr, "cannot read %s\n", argv[a]);
      return 2;
    }
    std::string group;
    while (in.word(group)) {
      g_case = in.word();
      std::printf("%s\n {", sep);
      sep = ",";
      g_sep = "";
      str("case", g_case);
      str("group", group);
      if (group == "tables") tables_case(in);
      else if (group == "seed") seed_case(in);
      else if (group == "links") links_case(in);
      else {
        std::fprintf(stderr, "unknown group %s\n", group.c_str());
        return 2;
      }
      std::printf("}");
    }
    std::fclose(in.f);
  }
  std::printf("\n], \"broken\": %d}\n", g_broken);
  return g_broken ? 1 : 0;
}
