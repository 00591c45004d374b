// md_cent.h — betweenness and closeness centrality of the residual layers on the device, and the
// pick of the reference's HBA / HCA baselines (baseline/HBA/hba_add.py, hba_2max.py
// critical_number, baseline/HCA/hca_add.py, hca_2max.py) from them.  Included by md_kernels.hip
// inside namespace md, after md_heur.h (whose key order heur_better the pick reuses).
//
// The graph of layer l is G_l: covered nodes and dead (covered / pruned) edges removed, isolated
// uncovered nodes kept; L = n - n_cov is the scripts' len(G).  The kernels read the HBM state the
// environment step leaves: rowptr / adj / calive, deg[l], the covered flags, GraphVar::n_cov.
//
//   md_cent_kernel        one workgroup per (source block, layer, graph): wave w runs the
//                         level-synchronous BFS of source 8 * block + w over the alive CSR entries,
//                         its distance / sigma / delta arrays private to the wave (LDS, or an HBM
//                         scratch slice for graphs too large).  A level is discovered by its
//                         predecessors marking distances (every writer stores the same value);
//                         every sum is then a pull in CSR row order by the lane that owns the
//                         node, so no sum depends on scheduling and nothing is accumulated with
//                         atomics:
//                           sigma(w) = sum over alive entries v of w's row with dist(v) = dist(w) - 1
//                           delta(v) = sum over alive entries w of v's row with dist(w) = dist(v) + 1
//                                      of sigma(v) * ((1 + delta(w)) / sigma(w))
//                         both sequentially from 0.0, every operation rounded on its own.
//                         Betweenness: the workgroup writes its block partial, per node the
//                         sequential sum from 0.0 of delta_s over its CENT_SRC_BLOCK sources in
//                         ascending order (s != node).  Closeness: a source's score is written
//                         directly, ((r - 1) / tot) * ((r - 1) / (L - 1)) from the integer reach r
//                         and distance sum tot (0.0 when tot == 0 or L <= 1).
//   md_cent_acc_kernel    betweenness: per node the running sum over the block partials in
//                         ascending block order (a launch round covers a range of blocks; the first
//                         round starts from 0.0).
//   md_cent_pick_kernel   scale (betweenness: one multiply by 1 / ((L - 1)(L - 2)) when L > 2),
//                         combine the layers (max, or one add), and the two-stage arg-max on
//                         (score bits, smallest id) over the live nodes; the pick is queued as the
//                         graph's pending action as md_heur_pick_kernel does.  With an output
//                         pointer it writes every node's two scaled scores instead.
//
// A source without an alive edge reaches nothing: its delta is 0.0 everywhere and its closeness
// 0.0, so its wave skips the search (x + 0.0 == x for the non-negative sums here).

constexpr int CENT_SRC_BLOCK = 8;                  // sources per block partial: one per wave
constexpr int CENT_THREADS = 64 * CENT_SRC_BLOCK;  // 512
constexpr int CENT_BETW = 0, CENT_CLOSE = 1;
constexpr int CENT_LDS_BYTES = 160000;             // dynamic LDS a workgroup may take (of 160 KiB)
constexpr int CENT_PICK_THREADS = 256;

typedef __attribute__((address_space(3))) unsigned long long lds_u64;

// bytes per node and wave of the search arrays: LDS keeps 16-bit distances, HBM scratch 32-bit
__host__ __device__ inline int cent_npad(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int cent_lds_node_bytes(int kind) { return kind == CENT_BETW ? 18 : 2; }
__host__ __device__ inline int cent_scr_node_bytes(int kind) { return kind == CENT_BETW ? 20 : 4; }
__host__ __device__ inline bool cent_fits_lds(int n, int kind) {
  return n < 65535 && (long long)cent_npad(n) * CENT_SRC_BLOCK * cent_lds_node_bytes(kind) <= CENT_LDS_BYTES;
}

struct CentArgs {
  double* part;         // betweenness: [workgroup of the launch][stride] block partials
  double* acc;          // [2][tot_n]: betweenness running sums / closeness scores
  unsigned char* scr;   // HBM search arrays, scr_wg bytes per workgroup; null: LDS
  long long scr_wg;
  int stride;           // row length of part (the largest n of the launch)
  int sb0;              // first source block of this round
  int kind;
  int tot_n;
};

// The wave-private search arrays.  Lanes of one wave exchange values through them between
// levels: relaxed atomic accesses (plain loads and stores in the ISA) and a fence per level.
struct CentLds {
  typedef lds_u64* PD;
  typedef lds_u16* PT;
  static constexpr unsigned INF = 0xffffu;
  static __device__ __forceinline__ double ld(PD a, int i) {
    return __longlong_as_double((long long)__hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT));
  }
  static __device__ __forceinline__ void st(PD a, int i, double v) {
    __hip_atomic_store(a + i, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
  static __device__ __forceinline__ unsigned ldd(PT a, int i) {
    return __hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
  static __device__ __forceinline__ void std_(PT a, int i, unsigned v) {
    __hip_atomic_store(a + i, (uint16_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
  static __device__ __forceinline__ void level_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
};
struct CentScr {
  typedef unsigned long long* PD;
  typedef unsigned* PT;
  static constexpr unsigned INF = 0xffffffffu;
  static __device__ __forceinline__ double ld(PD a, int i) {
    return __longlong_as_double((long long)__hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
  }
  static __device__ __forceinline__ void st(PD a, int i, double v) {
    __hip_atomic_store(a + i, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  static __device__ __forceinline__ unsigned ldd(PT a, int i) {
    return __hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  static __device__ __forceinline__ void std_(PT a, int i, unsigned v) {
    __hip_atomic_store(a + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  // (the wave's own stores have left before its lanes read them back)
  static __device__ __forceinline__ void level_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }
};

struct CentRows {  // one layer's residual CSR of a graph
  const int* rp;
  const int* adj;
  const uint8_t* ca;
  const int* deg;
  int n;
};

// One source's search on one wave.  Returns the deepest level; closeness: the reach (source
// included) and the distance sum in r_out / tot_out (valid in every lane).
template <class M, bool BETW>
__device__ __forceinline__ int cent_search(const CentRows& R, int s, typename M::PT dist, typename M::PD sigma,
                                           typename M::PD delta, long long* r_out, long long* tot_out) {
  const int lane = threadIdx.x & 63, n = R.n;
  for (int v = lane; v < n; v += 64) {
    M::std_(dist, v, v == s ? 0u : M::INF);
    if (BETW) {
      M::st(delta, v, 0.0);
      if (v == s) M::st(sigma, v, 1.0);
    }
  }
  M::level_fence();
  long long cnt = 0, tot = 0;
  unsigned d = 0;
  while (true) {
    // discover level d + 1: the nodes of level d mark their unvisited alive neighbours (every
    // writer stores the same value; a reader that still sees INF stores it again)
    for (int v0 = 0; v0 < n; v0 += 64) {
      const int v = v0 + lane;
      if (v >= n || M::ldd(dist, v) != d) continue;
      const int k1 = R.rp[v + 1];
      for (int k = R.rp[v]; k < k1; ++k) {
        const bool al = R.ca[k];
        const int w = R.adj[k];
        if (al && M::ldd(dist, w) == M::INF) M::std_(dist, w, d + 1);
      }
    }
    M::level_fence();
    // every node of the new level, by the lane that owns it: counted; betweenness: sigma pulled
    // over its row in CSR order (the discovery order above decides nothing)
    bool found = false;
    for (int v0 = 0; v0 < n; v0 += 64) {
      const int v = v0 + lane;
      if (v >= n || M::ldd(dist, v) != d + 1) continue;
      found = true;
      cnt += 1;
      tot += d + 1;
      if (BETW) {
        double sum = 0.0;
        const int k1 = R.rp[v + 1];
        for (int k = R.rp[v]; k < k1; ++k) {
          const bool al = R.ca[k];
          const int u = R.adj[k];
          if (al && M::ldd(dist, u) == d) sum = sum + M::ld(sigma, u);
        }
        M::st(sigma, v, sum);
      }
    }
    if (BETW) M::level_fence();
    if (__ballot(found) == 0ull) break;
    d += 1;
  }
  if (BETW) {
    // dependencies, deepest level first (level d's nodes have no successor: delta stays 0.0; the
    // source's own delta is not part of the sum over sources and stays 0.0 too)
    for (int dd = (int)d - 1; dd >= 1; --dd) {
      for (int v0 = 0; v0 < n; v0 += 64) {
        const int v = v0 + lane;
        if (v >= n || M::ldd(dist, v) != (unsigned)dd) continue;
        const double sv = M::ld(sigma, v);
        double a = 0.0;
        const int k1 = R.rp[v + 1];
        for (int k = R.rp[v]; k < k1; ++k) {
          const bool al = R.ca[k];
          const int w = R.adj[k];
          if (!al || M::ldd(dist, w) != (unsigned)dd + 1u) continue;
          const double coeff = (1.0 + M::ld(delta, w)) / M::ld(sigma, w);
          a = a + sv * coeff;
        }
        M::st(delta, v, a);
      }
      M::level_fence();
    }
  } else {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cnt += __shfl_xor(cnt, o, 64);
      tot += __shfl_xor(tot, o, 64);
    }
    *r_out = cnt + 1;
    *tot_out = tot;
  }
  return (int)d;
}

template <class M, bool BETW>
__device__ __forceinline__ void cent_block(const Params& p, const CentArgs& a, const GraphInfo& gi, int l, int sb,
                                           int wg, typename M::PT dist, typename M::PD sigma, typename M::PD delta,
                                           int npad, int* sh_active) {
  const int w = threadIdx.x >> 6, n = gi.n;
  CentRows R;
  // (selected, not indexed: a run-time index into the argument arrays would put them on the stack)
  R.rp = l ? p.rowptr[1] + gi.roff[1] : p.rowptr[0] + gi.roff[0];
  R.adj = l ? p.adj[1] + gi.coff[1] : p.adj[0] + gi.coff[0];
  R.ca = l ? p.calive[1] + gi.coff[1] : p.calive[0] + gi.coff[0];
  R.deg = (l ? p.deg[1] : p.deg[0]) + gi.node_off;
  R.n = n;
  const int s = sb * CENT_SRC_BLOCK + w;
  const bool active = s < n && R.deg[s] > 0 && !p.covered[gi.node_off + s];
  if ((threadIdx.x & 63) == 0) sh_active[w] = active ? 1 : 0;
  if (active) {
    long long r = 0, tot = 0;
    cent_search<M, BETW>(R, s, dist + (size_t)w * npad, sigma + (size_t)w * npad, delta + (size_t)w * npad, &r, &tot);
    if (!BETW && (threadIdx.x & 63) == 0) {
      const int L = n - p.gvar[gi.gidx].n_cov;
      double c = 0.0;
      if (tot != 0 && L > 1) c = (((double)r - 1.0) / (double)tot) * (((double)r - 1.0) / (double)(L - 1));
      a.acc[(size_t)l * a.tot_n + gi.node_off + s] = c;
    }
  }
  if (!BETW) return;
  __syncthreads();
  double* out = a.part + (size_t)wg * a.stride;
  for (int v = threadIdx.x; v < n; v += CENT_THREADS) {
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < CENT_SRC_BLOCK; ++k)
      if (sh_active[k]) sum = sum + M::ld(delta + (size_t)k * npad, v);
    out[v] = sum;
  }
}

// grid (source blocks of the round, 2 layers, graphs of the launch list)
__global__ void __launch_bounds__(CENT_THREADS) md_cent_kernel(Params p, CentArgs a) {
  __shared__ int sh_active[CENT_SRC_BLOCK];
  const GraphInfo gi = p.ginfo[p.glist[blockIdx.z]];
  const int l = blockIdx.y, sb = a.sb0 + (int)blockIdx.x;
  if (sb * CENT_SRC_BLOCK >= gi.n) return;  // (whole workgroup: before any barrier)
  const int wg = ((int)blockIdx.z * 2 + l) * (int)gridDim.x + (int)blockIdx.x;
  const int npad = cent_npad(gi.n);
  const size_t wn = (size_t)CENT_SRC_BLOCK * npad;
  if (a.scr == nullptr) {
    lds_u64* base = (lds_u64*)(unsigned long long*)lds_base();
    if (a.kind == CENT_BETW)
      cent_block<CentLds, true>(p, a, gi, l, sb, wg, (lds_u16*)(base + 2 * wn), base, base + wn, npad, sh_active);
    else
      cent_block<CentLds, false>(p, a, gi, l, sb, wg, (lds_u16*)base, base, base, npad, sh_active);
  } else {
    unsigned long long* base = (unsigned long long*)(a.scr + (size_t)wg * a.scr_wg);
    if (a.kind == CENT_BETW)
      cent_block<CentScr, true>(p, a, gi, l, sb, wg, (unsigned*)(base + 2 * wn), base, base + wn, npad, sh_active);
    else
      cent_block<CentScr, false>(p, a, gi, l, sb, wg, (unsigned*)base, base, base, npad, sh_active);
  }
}

// Betweenness: acc[l][v] (+)= the round's block partials in ascending block order.
// grid (node chunks, 2, graphs); rblocks: the source blocks per round (md_cent_kernel's gridDim.x).
__global__ void __launch_bounds__(CENT_PICK_THREADS) md_cent_acc_kernel(Params p, CentArgs a, int rblocks) {
  const GraphInfo gi = p.ginfo[p.glist[blockIdx.z]];
  const int l = blockIdx.y, v = blockIdx.x * CENT_PICK_THREADS + threadIdx.x;
  if (v >= gi.n) return;
  const int nsb = (gi.n + CENT_SRC_BLOCK - 1) / CENT_SRC_BLOCK;
  const int hi = min(a.sb0 + rblocks, nsb);
  double* dst = a.acc + (size_t)l * a.tot_n + gi.node_off + v;
  double s = a.sb0 == 0 ? 0.0 : *dst;
  const double* src = a.part + ((size_t)((int)blockIdx.z * 2 + l) * rblocks) * a.stride + v;
  for (int sb = a.sb0; sb < hi; ++sb) s = s + src[(size_t)(sb - a.sb0) * a.stride];
  if (a.sb0 < hi) *dst = s;
}

__device__ __forceinline__ double cent_scale(int kind, int L) {
  return kind == CENT_BETW && L > 2 ? 1.0 / (double)((long long)(L - 1) * (long long)(L - 2)) : 1.0;
}

// The pick over the finished sums: the structure of md_heur_pick_kernel (blocks [0, nb) of grid
// row y take graph glist[y]'s nodes grid-strided; the last block to arrive reduces the block
// partials and queues the pick), the key the bit pattern of the non-negative combined score.
// out != null: no pick; every node's scaled scores go to out[l][node] instead.
__global__ void __launch_bounds__(CENT_PICK_THREADS) md_cent_pick_kernel(Params p, const double* acc, double* out,
                                                                         long long* part, unsigned* ctr, int kind,
                                                                         int comb, int tot_n) {
  __shared__ long long sh_s[CENT_PICK_THREADS / 64];
  __shared__ int sh_i[CENT_PICK_THREADS / 64];
  __shared__ int sh_last;
  const int y = blockIdx.y, nb = gridDim.x;
  const GraphInfo gi = p.ginfo[p.glist[y]];
  const int* deg0 = p.deg[0] + gi.node_off;
  const int L = gi.n - p.gvar[gi.gidx].n_cov;
  const double scale = cent_scale(kind, L);
  const bool scaled = kind == CENT_BETW && L > 2;
  long long bs = 0;
  int bi = -1;
  for (int x = blockIdx.x * CENT_PICK_THREADS + threadIdx.x; x < gi.n; x += nb * CENT_PICK_THREADS) {
    double c0 = acc[gi.node_off + x], c1 = acc[(size_t)tot_n + gi.node_off + x];
    if (scaled) {
      c0 = c0 * scale;
      c1 = c1 * scale;
    }
    if (out != nullptr) {
      out[gi.node_off + x] = c0;
      out[(size_t)tot_n + gi.node_off + x] = c1;
      continue;
    }
    if (ldc(deg0 + x) <= 0) continue;
    const double c = comb == HEUR_MAX ? (c0 > c1 ? c0 : c1) : c0 + c1;
    const long long s = __double_as_longlong(c);
    if (bi < 0 || s > bs) {  // ascending x: the least id keeps a tie
      bs = s;
      bi = x;
    }
  }
  if (out != nullptr) return;
  auto reduce = [&](long long s, int id) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long s2 = __shfl_xor(s, o, 64);
      const int i2 = __shfl_xor(id, o, 64);
      if (heur_better(s2, i2, s, id)) {
        s = s2;
        id = i2;
      }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
      sh_s[threadIdx.x >> 6] = s;
      sh_i[threadIdx.x >> 6] = id;
    }
    __syncthreads();
    s = sh_s[0];
    id = sh_i[0];
    for (int w = 1; w < CENT_PICK_THREADS / 64; ++w)
      if (heur_better(sh_s[w], sh_i[w], s, id)) {
        s = sh_s[w];
        id = sh_i[w];
      }
    bs = s;
    bi = id;
  };
  reduce(bs, bi);
  long long* mine = part + 2 * ((size_t)y * nb + blockIdx.x);
  if (threadIdx.x == 0) {
    __hip_atomic_store(mine, bs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + 1, (long long)bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the agent-scope stores have left before the arrival is counted (as md_heur_pick_kernel)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    sh_last = __hip_atomic_fetch_add(ctr + y, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nb - 1;
  }
  __syncthreads();
  if (!sh_last) return;
  bs = 0;
  bi = -1;
  for (int b = threadIdx.x; b < nb; b += CENT_PICK_THREADS) {
    const long long* q = part + 2 * ((size_t)y * nb + b);
    const long long s2 = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int i2 = (int)__hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (heur_better(s2, i2, bs, bi)) {
      bs = s2;
      bi = i2;
    }
  }
  reduce(bs, bi);
  if (threadIdx.x == 0) {
    stc(p.pend + gi.node_off, bi);
    __hip_atomic_store(ctr + y, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
