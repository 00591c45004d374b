// md_heur.h — device rollouts of the reference's hand-written baselines (baseline/HDA/hda_2max.py,
// hda_add.py, baseline/CI/ci_max.py, ci_add.py of every variant directory), included by
// md_kernels.hip inside namespace md.
//
// A baseline rollout is the environment's own loop -- cover the pick, run the mutual-LMCC cascade
// (the scripts' MCC(G1, G2) is mcc_fixed_point) until the state is terminal (their ND_temp == 1) --
// with the pick taken from an integer score of the residual degrees instead of the network:
//   HDA   s_l(v) = d_l(v)
//   CI    s_l(v) = -1 if d_l(v) == 0, else (d_l(v) - 1) * sum over alive neighbours u of (d_l(u) - 1)
// combined over the layers as max(s_0, s_1) or s_0 + s_1; the live node (layer-0 residual degree
// > 0) of largest score is picked, the smallest id among equals (the scripts' stable
// sorted(..., reverse=True) over nodes in id order).
//
// Two paths:
//   md_heur_kernel       graphs whose environment fits LDS: one 512-thread workgroup per graph
//                        (persistent grid), the state staged once (env_stage_lds, the EnvView
//                        layout) and resident for the whole rollout; per step the residual degrees
//                        (and CI's neighbour sums) by edge-parallel LDS adds over the alive list,
//                        one block arg-max, the cover and the fixed point.  The state goes back to
//                        HBM once, at the end (what env_step writes per step).
//   md_heur_pick_kernel  graphs in HBM (too large for LDS, or MD_VARIANT=64): the pick alone,
//                        grid-strided over the nodes from deg[l] and the CSR; it queues the pick
//                        as the graph's pending action, and the host alternates it with the
//                        environment step launch (md_step's).
//
// Exactness: every score is a 64-bit integer.  The LDS path accumulates a node's neighbour sum in
// a 32-bit LDS word read as unsigned: at most 65535 neighbours of degree at most 65535
// (phase_a_fits_lds: n <= 65535) sum to at most 65534 * 65535 < 2^32.  The product with d - 1 and
// the sum of the two layers stay below 2^50.  The HBM path accumulates in 64 bits.

// Launch word of a heuristic launch (Params::sel_step, which only rollout launches with host
// selection read otherwise): kind | combine << 8.
__device__ __forceinline__ int heur_kind(int word) { return word & 0xff; }
__device__ __forceinline__ int heur_combine(int word) { return (word >> 8) & 0xff; }
constexpr int HEUR_HDA = 0, HEUR_CI = 1, HEUR_MAX = 0, HEUR_ADD = 1;

// The key order of every arg-max here: larger score first, then the smaller id; id < 0 = none.
__device__ __forceinline__ bool heur_better(long long s2, int i2, long long s, int i) {
  return i2 >= 0 && (i < 0 || s2 > s || (s2 == s && i2 < i));
}
__device__ __forceinline__ long long heur_score(int kind, int comb, int d0, int d1, unsigned ns0, unsigned ns1) {
  long long s0, s1;
  if (kind == HEUR_HDA) {
    s0 = d0;
    s1 = d1;
  } else {
    s0 = d0 == 0 ? -1ll : (long long)(d0 - 1) * (long long)ns0;
    s1 = d1 == 0 ? -1ll : (long long)(d1 - 1) * (long long)ns1;
  }
  return comb == HEUR_MAX ? (s0 > s1 ? s0 : s1) : s0 + s1;
}

struct HeurBest {
  long long s;
  int id;      // -1: no live node
  int sd0, sd1;  // degree sums per layer (2 x alive edges)
};
// Block arg-max on (score, smallest id) with the two degree sums: a wave butterfly, then one LDS
// exchange across the 8 waves.  Leading barrier only (as block_sum2).
__device__ __forceinline__ HeurBest heur_block_best(long long s, int id, int sd0, int sd1, int* tmp) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int lo2 = __shfl_xor((int)(unsigned)(unsigned long long)s, o, 64);
    const int hi2 = __shfl_xor((int)(unsigned)((unsigned long long)s >> 32), o, 64);
    const int i2 = __shfl_xor(id, o, 64);
    const long long s2 = (long long)(((unsigned long long)(unsigned)hi2 << 32) | (unsigned)lo2);
    if (heur_better(s2, i2, s, id)) {
      s = s2;
      id = i2;
    }
    sd0 += __shfl_xor(sd0, o, 64);
    sd1 += __shfl_xor(sd1, o, 64);
  }
  __syncthreads();
  lds_i32* t = (lds_i32*)tmp;  // 5 words per wave
  if (lane_id() == 0) {
    const int w = wave_id();
    t[5 * w + 0] = (int)(unsigned)(unsigned long long)s;
    t[5 * w + 1] = (int)(unsigned)((unsigned long long)s >> 32);
    t[5 * w + 2] = id;
    t[5 * w + 3] = sd0;
    t[5 * w + 4] = sd1;
  }
  __syncthreads();
  HeurBest b;
  b.s = 0;
  b.id = -1;
  b.sd0 = b.sd1 = 0;
#pragma unroll
  for (int w = 0; w < NTHREADS / 64; ++w) {
    const long long s2 = (long long)(((unsigned long long)(unsigned)t[5 * w + 1] << 32) | (unsigned)t[5 * w + 0]);
    const int i2 = t[5 * w + 2];
    if (heur_better(s2, i2, b.s, b.id)) {
      b.s = s2;
      b.id = i2;
    }
    b.sd0 += t[5 * w + 3];
    b.sd1 += t[5 * w + 4];
  }
  return b;
}

// One graph's whole baseline rollout on this workgroup, LDS-resident (the graph fits:
// phase_a_fits_lds, decided by the host).  Returns the device error code (0 = none).
__device__ __forceinline__ int heur_rollout_lds(KParams& p, int g, int kind, int comb) {
  float* const lds = lds_base();
  GraphVar& gv = *(GraphVar*)(lds + L_GV);
  int* const ia = (int*)(lds + L_W);
  const GraphInfo gi = p.ginfo[g];
  const int n = gi.n, e0 = gi.e[0], et = e0 + gi.e[1];
  __syncthreads();  // the previous graph of this workgroup is done with the area
  gv_load(p, g, &gv);
  // (this rollout changes the state without the grid-wide step's class labels: they go stale)
  if (threadIdx.x == 0 && p.lab_ok != nullptr) stc(p.lab_ok + gi.gidx, 0);
  const EnvView<false> E = env_view<false>(p, gi, ia);
  env_stage_lds(E, n);
  __syncthreads();
  int err = 0;
  if (!gv.s0_done) {
    // MvcEnv.s0's prune, left to this launch by md_reset_deferred (as env_step runs it)
    int pr[2];
    const int lm = mcc_fixed_point<false>(E, pr, nullptr, -1, nullptr);
    if (threadIdx.x == 0) {
      gv.removed[0] += pr[0];
      gv.removed[1] += pr[1];
      gv.max_rank = lm;
      gv.lmcc = lm;
      gv.s0_done = 1;
    }
    __syncthreads();
  }
  while (true) {
    // residual degrees (and CI's neighbour sums, in the parent arrays the fixed point leaves
    // free between calls) by edge-parallel LDS adds over the alive list
    for (int x = threadIdx.x; x < n; x += NTHREADS) {
      uf_store(E.deg0, x, 0);
      uf_store(E.deg1, x, 0);
      uf_store(E.par0, x, 0);
      uf_store(E.par1, x, 0);
    }
    __syncthreads();
    for_each_alive<false>(E, [&](int e, int u, int v) {
      auto d = e < e0 ? E.deg0 : E.deg1;
      uf_add(d, u, 1);
      uf_add(d, v, 1);
    });
    __syncthreads();
    if (kind == HEUR_CI) {
      for_each_alive<false>(E, [&](int e, int u, int v) {
        auto d = e < e0 ? E.deg0 : E.deg1;
        auto s = e < e0 ? E.par0 : E.par1;
        const int du = uf_load(d, u), dv = uf_load(d, v);
        uf_add(s, u, dv - 1);
        uf_add(s, v, du - 1);
      });
      __syncthreads();
    }
    long long bs = 0;
    int bi = -1, sd0 = 0, sd1 = 0;
    for (int x = threadIdx.x; x < n; x += NTHREADS) {  // ascending x: the least id keeps a tie
      const int d0 = uf_load(E.deg0, x), d1 = uf_load(E.deg1, x);
      sd0 += d0;
      sd1 += d1;
      if (d0 > 0) {
        const long long s = heur_score(kind, comb, d0, d1, (unsigned)uf_load(E.par0, x), (unsigned)uf_load(E.par1, x));
        if (bi < 0 || s > bs) {
          bs = s;
          bi = x;
        }
      }
    }
    const HeurBest b = heur_block_best(bs, bi, sd0, sd1, E.tmp);
    if (b.sd0 == 0 || b.sd1 == 0) break;  // terminal (U/mvc_env.py:128-131; the scripts' ND_temp == 1)
    const int a = b.id;
    if (a < 0 || a >= n) { err = ERR_LIVE_MISMATCH; break; }  // layer 1 alive, no layer-0 live node
    if (E.covered(a)) { err = ERR_COVERED; break; }
    __syncthreads();  // every thread has read covered(a) before it is set
    if (threadIdx.x == 0) {
      stc(E.gcov + a, (uint8_t)1);
      E.cov8[a] = 1;
    }
    __syncthreads();
    int pr[2], c[2];
    const int lm = mcc_fixed_point<false>(E, pr, nullptr, a, c);
    if (threadIdx.x == 0) {
      gv.counter[0] += c[0];
      gv.counter[1] += c[1];
      gv.removed[0] += pr[0];
      gv.removed[1] += pr[1];
      gv.n_cov += 1;
      gv.lmcc = lm;
      if (gv.steps < n) {
        stc(p.tr_action + gi.node_off + gv.steps, a);
        stc(p.tr_rank + gi.node_off + gv.steps, lm);
      }
      gv.steps += 1;
    }
    __syncthreads();
  }
  __syncthreads();
  // the final state to HBM, as env_step leaves it after a step: degrees, live list, aggregates,
  // q masked; the edges killed during the rollout (dead list) with their CSR flags
  const EnvAgg ag = env_features<false>(E, n, p.deg[0] + gi.node_off, p.deg[1] + gi.node_off,
                                        (float*)(p.live + 4 * (size_t)gi.node_off), p.q + gi.node_off);
  if (ag.bad && !err) err = ERR_LIVE_MISMATCH;
  __syncthreads();
  if (threadIdx.x == 0) {
    gv.n_live = ag.nlive;
    gv.dmax[0] = ag.dm0;
    gv.dmax[1] = ag.dm1;
    gv.alive[0] = ag.sd0 / 2;
    gv.alive[1] = ag.sd1 / 2;
    gv.twohop[0] = ag.th0;
    gv.twohop[1] = ag.th1;
    gv.npend = 0;
    gv.argmax = -1;
    gv.status = (ag.sd0 == 0 || ag.sd1 == 0) ? ST_TERMINAL : ST_PAUSED;
  }
  const int nd = E.hdr[1];
  for (int i = threadIdx.x; i < nd; i += NTHREADS) {
    const int e = E.dl[i];
    if (e >= et) continue;
    const int l = e < e0 ? 0 : 1, kk = e < e0 ? e : e - e0;
    stc(E.gst[l] + kk, (uint8_t)E.st[e]);
    stc(E.calive[l] + E.epos[l][2 * kk], (uint8_t)0);
    stc(E.calive[l] + E.epos[l][2 * kk + 1], (uint8_t)0);
  }
  __syncthreads();
  gv_store(p, g, &gv);
  trace_publish(p, gi, gv.steps);
  return err;
}

// Persistent grid: workgroup b runs graphs b, b + grid, ... of the launch list.
__global__ void __launch_bounds__(NTHREADS, 1) md_heur_kernel(Params p, const float* __restrict__ wimg) {
  if (!kargs_layout_ok()) {
    if (threadIdx.x == 0) __hip_atomic_store(p.err, ERR_ABI, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  (void)wimg;
  KParams& kpp = kp();
  const int kind = heur_kind(kpp.sel_step), comb = heur_combine(kpp.sel_step);
  for (int i = blockIdx.x; i < kpp.nglist; i += gridDim.x) {
    const int err = heur_rollout_lds(kpp, kpp.glist[i], kind, comb);
    if (err) {
      if (threadIdx.x == 0) raise_err(kpp, err);
      break;
    }
  }
}

// ------------------------------------------------------------------ the pick over the HBM state
// One launch per removal: blocks [0, nb) of grid row y score graph glist[y]'s nodes grid-strided
// from the residual degrees the last environment step left in deg[l] (CI: the alive CSR entries
// of the node's rows), reduce to one partial per block, and the last block to finish a graph
// reduces the partials and queues the pick as the graph's pending action (pend[node_off]; -1:
// no live node).  part: [graphs][nb][2] i64 {score, id}; ctr: [graphs], left zero.
constexpr int HEUR_PICK_THREADS = 256;
__global__ void __launch_bounds__(HEUR_PICK_THREADS) md_heur_pick_kernel(Params p, long long* part, unsigned* ctr,
                                                                         int kind, int comb) {
  __shared__ long long sh_s[HEUR_PICK_THREADS / 64];
  __shared__ int sh_i[HEUR_PICK_THREADS / 64];
  __shared__ int sh_last;
  const int y = blockIdx.y, nb = gridDim.x;
  const GraphInfo gi = p.ginfo[p.glist[y]];
  const int* deg0 = p.deg[0] + gi.node_off;
  const int* deg1 = p.deg[1] + gi.node_off;
  long long bs = 0;
  int bi = -1;
  for (int x = blockIdx.x * HEUR_PICK_THREADS + threadIdx.x; x < gi.n; x += nb * HEUR_PICK_THREADS) {
    const int d0 = ldc(deg0 + x), d1 = ldc(deg1 + x);
    if (d0 <= 0) continue;
    long long s;
    if (kind == HEUR_HDA) {
      s = comb == HEUR_MAX ? (long long)max(d0, d1) : (long long)d0 + d1;
    } else {
      long long sl[2];
      for (int l = 0; l < 2; ++l) {
        const int d = l ? d1 : d0;
        const int* dg = l ? deg1 : deg0;
        const int* rp = p.rowptr[l] + gi.roff[l];
        const int* adj = p.adj[l] + gi.coff[l];
        const uint8_t* ca = p.calive[l] + gi.coff[l];
        long long ns = 0;
        for (int k = rp[x]; k < rp[x + 1]; ++k)
          if (ldc(ca + k)) ns += ldc(dg + adj[k]) - 1;
        sl[l] = d == 0 ? -1ll : (long long)(d - 1) * ns;
      }
      s = comb == HEUR_MAX ? (sl[0] > sl[1] ? sl[0] : sl[1]) : sl[0] + sl[1];
    }
    if (bi < 0 || s > bs) {  // ascending x: the least id keeps a tie
      bs = s;
      bi = x;
    }
  }
  auto reduce = [&](long long s, int id) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int lo2 = __shfl_xor((int)(unsigned)(unsigned long long)s, o, 64);
      const int hi2 = __shfl_xor((int)(unsigned)((unsigned long long)s >> 32), o, 64);
      const int i2 = __shfl_xor(id, o, 64);
      const long long s2 = (long long)(((unsigned long long)(unsigned)hi2 << 32) | (unsigned)lo2);
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
    for (int w = 1; w < HEUR_PICK_THREADS / 64; ++w)
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
    // the agent-scope stores have left before the arrival is counted: the partial is visible to
    // the block that sees it (which reads with agent-scope loads)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    sh_last = __hip_atomic_fetch_add(ctr + y, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nb - 1;
  }
  __syncthreads();
  if (!sh_last) return;
  bs = 0;
  bi = -1;
  for (int b = threadIdx.x; b < nb; b += HEUR_PICK_THREADS) {  // ascending blocks hold ascending ids per stride only:
    const long long* q = part + 2 * ((size_t)y * nb + b);       // the key order decides, not the visiting order
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
