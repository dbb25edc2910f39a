// Symbolic LDLᵀ, the ordering: nested dissection on the graph of the matrix with (constrained) minimum-degree leaves,
// hubs set aside and eliminated last (ldlt_symbolic.hpp has the why).
#include "ldlt_symbolic_detail.hpp"

#include "setup_threads.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <thread>
#include <unordered_map>

namespace slpx::ldlt_detail {

namespace {

// the graph of the matrix: neighbours of v = idx[ptr[v] .. ptr[v + 1]), ascending, no duplicates
struct Adj {
  std::vector<int32_t> ptr, idx;
  struct Range {
    const int32_t *b, *e;
    const int32_t* begin() const { return b; }
    const int32_t* end() const { return e; }
    size_t size() const { return static_cast<size_t>(e - b); }
  };
  Range operator[](int32_t v) const { return {idx.data() + ptr[v], idx.data() + ptr[v + 1]}; }
  size_t size() const { return ptr.size() - 1; }
};

// ---------------------------------------------------------------------------
// Ordering: nested dissection with (constrained) minimum-degree leaves
// ---------------------------------------------------------------------------
struct Orderer {
  const Adj& adj;
  const std::vector<uint8_t>& has_diag;
  const LdltOptions& opt;
  std::vector<int32_t> stamp, dist;
  // The two sides of a separator are dissected on two threads (down to a few levels: parallel_depth): they
  // share no node and no edge, every call marks its nodes with a stamp of its own, and what the sides do
  // share — the `avail` counts of the separator nodes above them, which both add to and nobody reads before
  // both are through — is updated atomically.  The order is the sequential one: left, right, separator.
  std::atomic<int32_t> cur_stamp{0};
  int32_t new_stamp() { return cur_stamp.fetch_add(1, std::memory_order_relaxed) + 1; }
  std::vector<int32_t> order;
  // Pairing state for nodes whose unregularized diagonal is structurally zero
  // (constraint rows, variables that appear only linearly): such a node z may only be
  // eliminated after an ORIGINAL neighbour v that no other zero-diagonal node has
  // already claimed — then its pivot is -a_zv^2/d_v.  Two zero-diagonal nodes claiming
  // the same v would make the leading block [[d,a,b],[a,0,0],[b,0,0]] singular whatever
  // the values.  With distinct claims the claimed pairs form paths whose every prefix
  // has a perfect matching, so every leading principal block is structurally
  // nonsingular.
  std::vector<uint8_t> gone, claimed;
  std::vector<int32_t> avail;  // # eliminated, unclaimed original neighbours
  std::atomic<bool> forced{false};  // some node had to be eliminated without a partner
  int parallel_depth = 0;
  size_t parallel_min_nodes = 1500;

  Orderer(const Adj& a, const std::vector<uint8_t>& hd, const LdltOptions& o)
      : adj(a), has_diag(hd), opt(o), stamp(a.size(), 0), dist(a.size(), 0),
        gone(a.size(), 0), claimed(a.size(), 0), avail(a.size(), 0) {
    unsigned t = SetupPool::get().threads();
    while (t > 1) {
      ++parallel_depth;
      t >>= 1;
    }
  }

  bool ready(int32_t v) const { return !opt.defer_constraints || has_diag[v] || avail[v] > 0; }

  void eliminate(int32_t v, std::vector<int32_t>& out) {
    if (opt.defer_constraints && !has_diag[v]) {
      // claim the partner that the fewest other waiting zero-diagonal nodes could use
      int32_t partner = -1, partner_demand = 0;
      for (int32_t w : adj[v]) {
        if (!gone[w] || claimed[w]) continue;
        int32_t demand = 0;
        for (int32_t u : adj[w])
          if (!gone[u] && u != v && !has_diag[u]) ++demand;
        if (partner < 0 || demand < partner_demand) {
          partner = w;
          partner_demand = demand;
        }
      }
      if (partner < 0) {
        forced.store(true, std::memory_order_relaxed);
      } else {
        claimed[partner] = 1;
        for (int32_t u : adj[partner]) __atomic_fetch_sub(&avail[u], 1, __ATOMIC_RELAXED);
      }
    }
    gone[v] = 1;
    out.push_back(v);
    for (int32_t u : adj[v]) __atomic_fetch_add(&avail[u], 1, __ATOMIC_RELAXED);
  }

  // Minimum degree on the subgraph induced by `nodes`; with defer_constraints a
  // zero-diagonal node is only eligible while it has an unclaimed eliminated partner.
  void min_degree(const std::vector<int32_t>& nodes, std::vector<int32_t>& out) {
    const int m = static_cast<int>(nodes.size());
    if (m <= 64) {
      // the usual case (a dissection leaf): neighbour sets as bit masks, membership through a stamp of the leaf's own
      const int32_t s = new_stamp();
      for (int i = 0; i < m; ++i) {
        stamp[nodes[i]] = s;
        dist[nodes[i]] = i;  // (position in the leaf: dist is free once a set is down to a leaf)
      }
      uint64_t a[64];
      for (int i = 0; i < m; ++i) {
        uint64_t bits = 0;
        for (int32_t w : adj[nodes[i]])
          if (stamp[w] == s) bits |= 1ull << dist[w];
        a[i] = bits;
      }
      uint64_t done = 0;
      for (int step = 0; step < m; ++step) {
        int best = -1, best_deg = 0;
        for (int pass = 0; pass < 2 && best < 0; ++pass)
          for (int i = 0; i < m; ++i) {
            if (((done >> i) & 1) || (pass == 0 && !ready(nodes[i]))) continue;
            const int deg = __builtin_popcountll(a[i]);
            if (best < 0 || deg < best_deg) {
              best = i;
              best_deg = deg;
            }
          }
        done |= 1ull << best;
        eliminate(nodes[best], out);
        const uint64_t nb = a[best];
        for (uint64_t rest = nb; rest != 0; rest &= rest - 1) {
          const int u = __builtin_ctzll(rest);
          a[u] = (a[u] | nb) & ~((1ull << u) | (1ull << best));
        }
        a[best] = 0;
      }
      return;
    }
    std::unordered_map<int32_t, int32_t> loc;
    loc.reserve(m * 2);
    for (int i = 0; i < m; ++i) loc[nodes[i]] = i;
    std::vector<std::vector<int32_t>> a(m);
    for (int i = 0; i < m; ++i)
      for (int32_t w : adj[nodes[i]]) {
        auto it = loc.find(w);
        if (it != loc.end()) a[i].push_back(it->second);
      }
    for (auto& v : a) std::sort(v.begin(), v.end());
    std::vector<uint8_t> done(m, 0);
    std::vector<int32_t> merged;
    for (int step = 0; step < m; ++step) {
      int best = -1;
      for (int pass = 0; pass < 2 && best < 0; ++pass)
        for (int i = 0; i < m; ++i) {
          if (done[i] || (pass == 0 && !ready(nodes[i]))) continue;
          if (best < 0 || a[i].size() < a[best].size()) best = i;
        }
      done[best] = 1;
      eliminate(nodes[best], out);
      for (int32_t u : a[best]) {
        merged.clear();
        std::set_union(a[u].begin(), a[u].end(), a[best].begin(), a[best].end(),
                       std::back_inserter(merged));
        merged.erase(std::remove_if(merged.begin(), merged.end(),
                                    [&](int32_t w) { return w == u || w == best; }),
                     merged.end());
        a[u].swap(merged);
      }
      a[best].clear();
    }
  }

  // Separator nodes: variables with a diagonal first, then zero-diagonal nodes as they
  // find partners.
  void order_separator(std::vector<int32_t> sep, std::vector<int32_t>& out) {
    std::sort(sep.begin(), sep.end());
    std::vector<uint8_t> done(sep.size(), 0);
    for (size_t step = 0; step < sep.size(); ++step) {
      int best = -1;
      for (int pass = 0; pass < 3 && best < 0; ++pass)
        for (size_t i = 0; i < sep.size() && best < 0; ++i) {
          if (done[i]) continue;
          const int32_t v = sep[i];
          if (pass == 0 ? (has_diag[v] != 0) : (pass == 1 ? ready(v) : true)) best = static_cast<int>(i);
        }
      done[best] = 1;
      eliminate(sep[best], out);
    }
  }

  // BFS inside the current subset (marked by stamp == s): the nodes in visiting order, and where each level starts
  struct Levels {
    std::vector<int32_t> nodes, ptr;  // level l = nodes[ptr[l] .. ptr[l + 1])
    size_t size() const { return ptr.size() - 1; }
    size_t count(size_t l) const { return static_cast<size_t>(ptr[l + 1] - ptr[l]); }
    const int32_t* begin(size_t l) const { return nodes.data() + ptr[l]; }
    const int32_t* end(size_t l) const { return nodes.data() + ptr[l + 1]; }
  };
  void bfs_levels(int32_t start, int32_t s, size_t expected, Levels& L) {
    L.nodes.clear();
    L.ptr.clear();
    L.nodes.reserve(expected);
    const int32_t visited = new_stamp();
    dist[start] = visited;
    L.nodes.push_back(start);
    L.ptr.push_back(0);
    size_t lo = 0;
    while (lo < L.nodes.size()) {
      const size_t hi = L.nodes.size();
      L.ptr.push_back(static_cast<int32_t>(hi));
      for (size_t q = lo; q < hi; ++q)
        for (int32_t w : adj[L.nodes[q]])
          if (stamp[w] == s && dist[w] != visited) {
            dist[w] = visited;
            L.nodes.push_back(w);
          }
      lo = hi;
    }
  }

  void dissect(std::vector<int32_t> nodes, std::vector<int32_t>& out, int depth = 0) {
    if (nodes.empty()) return;
    if (static_cast<int>(nodes.size()) <= opt.leaf_size) {
      min_degree(nodes, out);
      return;
    }
    const int32_t s = new_stamp();
    for (int32_t v : nodes) stamp[v] = s;
    // pseudo-peripheral start: two BFS sweeps
    Levels levels;
    bfs_levels(nodes[0], s, nodes.size(), levels);
    const size_t reached = levels.nodes.size();
    if (reached < nodes.size()) {
      // disconnected: order each component on its own
      std::vector<int32_t> comp, rest;
      const int32_t mark = new_stamp();
      for (int32_t v : levels.nodes) {
        dist[v] = mark;
        comp.push_back(v);
      }
      for (int32_t v : nodes)
        if (dist[v] != mark) rest.push_back(v);
      dissect(std::move(comp), out, depth);
      dissect(std::move(rest), out, depth);
      return;
    }
    for (int sweep = 0; sweep < 2; ++sweep) {
      const int32_t far = *levels.begin(levels.size() - 1);
      bfs_levels(far, s, nodes.size(), levels);
    }
    if (levels.size() < 3) {
      min_degree(nodes, out);
      return;
    }
    // separator level: balance the two sides
    size_t total = nodes.size(), acc = 0, best_m = 1;
    size_t best_gap = total;
    for (size_t m = 0; m + 1 < levels.size(); ++m) {
      if (m >= 1) {
        size_t left = acc, right = total - acc - levels.count(m);
        size_t gap = left > right ? left - right : right - left;
        if (gap < best_gap) {
          best_gap = gap;
          best_m = m;
        }
      }
      acc += levels.count(m);
    }
    // shrink the separator to the nodes that actually touch the next level
    const int32_t nextmark = new_stamp();
    for (const int32_t* v = levels.begin(best_m + 1); v != levels.end(best_m + 1); ++v) dist[*v] = nextmark;
    std::vector<int32_t> sep, left, right;
    left.reserve(static_cast<size_t>(levels.ptr[best_m + 1]));
    for (const int32_t* pv = levels.begin(best_m); pv != levels.end(best_m); ++pv) {
      const int32_t v = *pv;
      bool touches = false;
      for (int32_t w : adj[v])
        if (stamp[w] == s && dist[w] == nextmark) {
          touches = true;
          break;
        }
      (touches ? sep : left).push_back(v);
    }
    left.insert(left.end(), levels.nodes.begin(), levels.nodes.begin() + levels.ptr[best_m]);
    right.assign(levels.nodes.begin() + levels.ptr[best_m + 1], levels.nodes.end());
    std::sort(left.begin(), left.end());
    std::sort(right.begin(), right.end());
    if (std::getenv("SLPX_ND_DEBUG")) std::fprintf(stderr, "nd depth %d: %zu nodes, %zu levels, sep %zu left %zu right %zu\n", depth, nodes.size(), levels.size(), sep.size(), left.size(), right.size());
    if (depth < parallel_depth && std::min(left.size(), right.size()) >= parallel_min_nodes) {
      std::vector<int32_t> right_out;
      std::exception_ptr failed;
      std::thread other([&] {
        try {
          dissect(std::move(right), right_out, depth + 1);
        } catch (...) {
          failed = std::current_exception();
        }
      });
      try {
        dissect(std::move(left), out, depth + 1);
      } catch (...) {
        other.join();
        throw;
      }
      other.join();
      if (failed) std::rethrow_exception(failed);
      out.insert(out.end(), right_out.begin(), right_out.end());
    } else {
      dissect(std::move(left), out, depth);
      dissect(std::move(right), out, depth);
    }
    // separator last
    order_separator(std::move(sep), out);
  }
};

// (the pattern holds each pair once, below the diagonal: no duplicates to remove)
Adj adjacency(const CscPattern& lower) {
  const int n = lower.cols;
  Adj adj;
  adj.ptr.assign(n + 1, 0);
  for (int c = 0; c < n; ++c)
    for (int p = lower.colptr[c]; p < lower.colptr[c + 1]; ++p) {
      const int r = lower.rowidx[p];
      if (r != c) {
        ++adj.ptr[r + 1];
        ++adj.ptr[c + 1];
      }
    }
  for (int v = 0; v < n; ++v) adj.ptr[v + 1] += adj.ptr[v];
  adj.idx.resize(adj.ptr[n]);
  std::vector<int32_t> next(adj.ptr.begin(), adj.ptr.end() - 1);
  for (int c = 0; c < n; ++c)
    for (int p = lower.colptr[c]; p < lower.colptr[c + 1]; ++p) {
      const int r = lower.rowidx[p];
      if (r != c) {
        adj.idx[next[r]++] = c;
        adj.idx[next[c]++] = r;
      }
    }
  bool dup = false;
  for (int v = 0; v < n; ++v) {
    int32_t* b = adj.idx.data() + adj.ptr[v];
    int32_t* e = adj.idx.data() + adj.ptr[v + 1];
    if (!std::is_sorted(b, e)) std::sort(b, e);
    dup = dup || std::adjacent_find(b, e) != e;
  }
  if (dup) {  // (a pattern that names an entry twice: compact the lists)
    std::vector<int32_t> ptr2(n + 1, 0), idx2;
    for (int v = 0; v < n; ++v) {
      int32_t* b = adj.idx.data() + adj.ptr[v];
      int32_t* e = std::unique(b, adj.idx.data() + adj.ptr[v + 1]);
      idx2.insert(idx2.end(), b, e);
      ptr2[v + 1] = static_cast<int32_t>(idx2.size());
    }
    adj.ptr.swap(ptr2);
    adj.idx.swap(idx2);
  }
  return adj;
}

// Hubs (LdltOptions::hub_factor) defeat level-set dissection — everything is two steps from
// everything — so they are taken out of the graph that is dissected and eliminated last.
void split_hubs(const Adj& adj, const LdltOptions& opt, std::vector<int32_t>& rest, std::vector<int32_t>& hubs) {
  const int n = static_cast<int>(adj.size());
  std::vector<size_t> degs(n);
  for (int v = 0; v < n; ++v) degs[v] = adj[v].size();
  std::vector<size_t> sorted = degs;
  std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
  const size_t median = n ? sorted[n / 2] : 0;
  const size_t hub_degree =
      std::max<size_t>(opt.hub_floor, static_cast<size_t>(opt.hub_factor * static_cast<double>(median)));
  for (int v = 0; v < n; ++v) (degs[v] > hub_degree ? hubs : rest).push_back(v);
}

}  // namespace

void order_columns(const CscPattern& lower, const LdltOptions& opt, const std::vector<int32_t>* user_perm, Elimination& E,
                   SetupLap& lap) {
  const int n = E.n;
  if (user_perm != nullptr && !user_perm->empty()) {
    E.perm = *user_perm;
  } else {
    const Adj adj = adjacency(lower);
    lap("  ldlt:   adjacency");
    Orderer ord(adj, E.has_diag, opt);
    std::vector<int32_t> rest, hubs;
    split_hubs(adj, opt, rest, hubs);
    ord.order.reserve(n);
    lap("  ldlt:   hubs");
    ord.dissect(std::move(rest), ord.order);
    lap("  ldlt:   dissect");
    if (!hubs.empty()) ord.order_separator(std::move(hubs), ord.order);
    E.perm = std::move(ord.order);
    E.ordering_forced = ord.forced.load();
  }
  if (static_cast<int>(E.perm.size()) != n) throw std::runtime_error("ldlt: bad permutation size");
  E.iperm.assign(n, -1);
  for (int k = 0; k < n; ++k) E.iperm[E.perm[k]] = k;
  for (int k = 0; k < n; ++k)
    if (E.iperm[k] < 0) throw std::runtime_error("ldlt: permutation is not a bijection");
}

}  // namespace slpx::ldlt_detail
