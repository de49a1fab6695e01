// sgm_sweep_rows.inc — the row sweeps of the SGM mode, included by sgm_sweep.hip once per cost source (the description is there):
//   JN_SW_ROWS = k_sw_w,  JN_SW_VOL = false: the costs are the 1x3 SAD of the prefiltered rows `src` (include/jn_sgm.h);
//   JN_SW_ROWS = k_swc_w, JN_SW_VOL = true:  they are read from the byte volume `src` [n][H][W][D], natural column order, d ascending
//                                            (include/jn_sgm_cost.h).
// Only the cost source differs: everything behind Cp[] is the same text.  (Two kernels from one text and not a __device__ template under two
// wrappers: behind a wrapper the existing D = 64 forms took 8 more registers and the D = 256 final sweeps spilled 8 more.)
template <int NR, int NS, int RING, bool FINAL, bool WIDE, int LQ>
__global__ void __launch_bounds__(NS * 64, NR == 16 ? 3 : (NR == 32 && !FINAL) ? 2 : 1) JN_SW_ROWS(SwDev s, int n, int flip, const uint8_t* __restrict__ src, uint8_t* __restrict__ volF,
                                                  const uint8_t* __restrict__ volH0, const uint8_t* __restrict__ volH1, uint32_t* __restrict__ gx,
                                                  uint32_t* __restrict__ ctr, uint32_t* __restrict__ gminR, uint32_t* __restrict__ dLp) {
  constexpr bool VOL = JN_SW_VOL;
  const uint8_t* __restrict__ const gm = src;                   // what `src` is when !VOL ...
  const uint8_t* __restrict__ const cost = src;                 // ... and when VOL
  constexpr int NQ = LQ, PX = 64 / LQ;                         // lanes per pixel (4, or 8 for D = 256: 16 disparity pairs per lane either way), pixels per strip
  constexpr bool LATE_PROD = FINAL && LQ == 8;                 // where the last strip requests its producer block's columns (see there)
  constexpr int DPL = 2 * NR, SLOT = 3 * NQ * NR, BLK = NS * PX, MR = PX + DPL;
  constexpr int PW = LQ == 4 ? 4 : 2, NP = SLOT / PW, NG = (NP + 63) / 64;       // dwords per piece of a row of columns between blocks, pieces per row, pieces per lane
  typedef Piece<PW> Px;
  typedef typename Px::T piece_t;
  static_assert((RING & (RING - 1)) == 0, "ring depth is a power of two");
  __shared__ __attribute__((aligned(16))) uint32_t ring[RING][NS][SLOT];                    // boundary columns [row mod RING][strip][V0 | M0 | M1][quarter][NR]
  __shared__ __attribute__((aligned(16))) uint32_t nextblk[SLOT];                           // the next block's columns for the last strip (written and read by that wave only)
  __shared__ uint32_t minR[FINAL ? NS : 1][FINAL ? 2 : 1][FINAL ? NQ : 1][FINAL ? MR : 1];   // right-image winners of one row of one strip, per disparity quarter (rows alternate)
  __shared__ uint32_t minR_trash[FINAL ? NS : 1][FINAL ? NQ : 1][FINAL ? MR : 1];              // where lanes outside the image send theirs
  __shared__ int prog[NS], cons[NS];                           // rows published by strip w / rows of strip w's columns consumed by strip w-1
  __shared__ int s_ticket;
  extern __shared__ uint16_t sS[];                             // FINAL + sub-pixel: S of the block's pixels [BLK][D]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W = s.W, H = s.H, D = s.D, NB = s.NB;
  const uint32_t P2pk = (uint32_t)s.P2 * 0x10001u;
  const uint32_t tagpk = (((uint32_t)s.epoch & 0xFFu) << 8) | (((uint32_t)s.epoch >> 8) << 24);
  if (tid == 0) s_ticket = (int)atomicAdd(ctr, 1u);
  for (int k = tid; k < RING * NS * SLOT; k += NS * 64) (&ring[0][0][0])[k] = P2pk;            // X = P2: a path that starts here
  if (FINAL) for (int k = tid; k < NS * 2 * NQ * MR; k += NS * 64) (&minR[0][0][0][0])[k] = 0xFFFFFFFFu;
  __syncthreads();
  const int ticket = __builtin_amdgcn_readfirstlane(s_ticket);     // wave-uniform, and known to be: everything derived from it (frame, block, rows) stays scalar
  // producers (larger j) hold the smaller tickets; the block index is the major order: all frames walk through their parallelogram in phase
  // and finish together (frame-major tickets were measured: 2 588 against 3 168 pairs/s — the last frames run alone at the end)
  const int j = NB - 1 - ticket / n, frame = ticket % n;
  const int x0 = s.xmin + BLK * j;                             // sheared origin of this block: x' in [x0, x0 + BLK)
  const int ybs = max(0, -(x0 + BLK - 1)), ybe = min(H - 1, W - 1 - x0);
  if (ybs > ybe) return;
  if (tid < NS) { prog[tid] = ybs; cons[tid] = ybs - 1; }       // rows < prog published (row ybs - 1 = the initial fill); rows < cons read by the left neighbour
  __syncthreads();                                             // the only barriers of the kernel: before the first row
  uint32_t* my_gx = gx + ((size_t)frame * NB + j) * H * (size_t)SLOT;
  // the producer block (j + 1) and the rows it works on
  const bool has_prod = j + 1 < NB;
  const int x0p = x0 + BLK;
  const int ybsp = max(0, -(x0p + BLK - 1)), ybep = min(H - 1, W - 1 - x0p);
  const uint32_t* p_gx = gx + ((size_t)frame * NB + j + 1) * H * (size_t)SLOT;
  const bool last = wave == NS - 1;
  // The columns cross between blocks in 16-BYTE pieces (round 5; they were single dwords): a write-through dword store is one fabric write
  // of its own and costs ~6x a 16-byte store's time per byte, an 8-byte one 2.7x (MI355X_MICROARCH.md, stores of each flavour).  Every dword
  // still carries its tag, so nothing is assumed about how a wider store becomes visible.  Lanes beyond the row's NP pieces: the buffer's range
  // check drops their stores and returns zeros to their loads (they count as valid).  (Eight lanes per pixel: 8-byte pieces — as many
  // registers as the dwords took; with 16-byte ones the final sweep spills a dozen more.)
  piece_t g[NG];                                               // last strip: the producer's row, loaded a row ahead of its use
#pragma unroll
  for (int k = 0; k < NG; k++) g[k] = Px::zero();
  auto gx_rsrc = [&](const uint32_t* row) __attribute__((always_inline)) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(row), 0, SLOT * 4, 0x00020000);
  };
  auto load_prod = [&](int yr, piece_t (&dst)[NG]) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t r = gx_rsrc(p_gx + (size_t)yr * SLOT);     // wave-uniform
    int ln = lane;
    asm volatile("" : "+v"(ln));                                // scalar base + lane offset, formed here: a per-lane 64-bit pointer kept across the loop is two registers the final sweep lacks
#pragma unroll
    for (int k = 0; k < NG; k++) dst[k] = Px::load(r, 4 * PW * (ln + 64 * k));
  };
  auto tags_ok = [&](const piece_t (&v)[NG]) __attribute__((always_inline)) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < NG; k++) ok = ok && (Px::all_tagged(v[k], tagpk) || (NP % 64 != 0 && lane + 64 * k >= NP));
    return ok;
  };
  auto to_nextblk = [&](const piece_t (&v)[NG], uint32_t* nb) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NG; k++) {
      const int o = lane + 64 * k;
      if (NP % 64 == 0 || o < NP) *reinterpret_cast<piece_t*>(nb + PW * o) = v[k] & 0x00FF00FFu;
    }
  };
  const int q = lane / PX, p = lane & (PX - 1);
  const int xl = x0 + PX * wave + p;                           // this lane's sheared column
  const uint32_t P1pk = (uint32_t)s.P1 * 0x10001u;
  uint32_t V[NR], G[NR], M[NR];                                // X of the pixel this lane computed last, per path: vertical, own diagonal, other diagonal
#pragma unroll
  for (int r = 0; r < NR; r++) V[r] = G[r] = M[r] = P2pk;
  const size_t img_rows = (size_t)H * s.Wp;
  // A ROW'S INPUT BYTES travel through LDS.  The lanes of a strip read overlapping windows of the same ~150 bytes of the right row (and 19 of
  // the left one): loaded per lane into registers a row ahead — 17 loop-carried registers that the final sweep had no room for — they are now
  // fetched ONCE per wave (8 bytes per lane), two rows ahead, and read from LDS right before the costs.  A lane's window starts at byte
  // p + DPL q: any alignment, and a misaligned ds_read costs 64 cycles of the CU's LDS pipeline against 4.6 for an aligned one
  // (scripts/probes/lds_unaligned_probe.hip).  The fetching lanes therefore store FOUR copies of the row, shifted by 0 .. 3 bytes
  // (v_alignbyte of their two dwords), and a lane reads dword-aligned from copy p & 3.  Two rows of LDS per strip: the commit of row yb + 2
  // overwrites row yb's slot behind row yb's reads (LDS serves a wave's instructions in order).
  constexpr int RBYTES = PX - 1 + DPL * (NQ - 1) + 4 * (NR / 2 - 1) + 8;      // right-row bytes a strip touches
  constexpr int NRD = (RBYTES + 3) / 4, NLD = (PX + 6) / 4, TD = NRD + NLD, NSTG = (TD + 63) / 64, RS = (TD + 3) & ~3;
  __shared__ uint32_t rowbuf[NS][2][4][RS];                     // [strip][row parity][byte shift][dword]
  const int y0 = flip ? H - 1 - ybs : ybs;
  const long long row_step = (flip ? -(long long)s.Wp : (long long)s.Wp) + 1;
  const uint8_t* gsrc;                                          // left row of the strip's next fetch (wave-uniform; the right image lies n images further)
  uint32_t soff[NSTG];                                          // this lane's dword of a fetch, relative to gsrc
  {
    gsrc = gm + (size_t)frame * img_rows + (size_t)y0 * s.Wp + s.padl - 1 + (x0 + PX * wave + ybs);
    const uint32_t to_right = (uint32_t)((size_t)n * img_rows);
#pragma unroll
    for (int k = 0; k < NSTG; k++) { const int i = lane + 64 * k; soff[k] = i < NRD ? to_right + 4 * i : 4 * (min(i, TD - 1) - NRD); }
  }
  int next_row = ybs;                                           // the row the next fetch is for (rows beyond ybe fetch ybe again: unconditional loads)
  auto stage_load = [&](uint64_t (&d)[NSTG]) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NSTG; k++) d[k] = load_u64_unaligned(gsrc + soff[k]);
    gsrc += next_row < ybe ? row_step : 0;
    next_row++;
  };
  auto stage_write = [&](int row, const uint64_t (&d)[NSTG]) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NSTG; k++) {
      const uint32_t lo = (uint32_t)d[k], hi = (uint32_t)(d[k] >> 32);
      if (TD % 64 != 0 && lane + 64 * k >= TD) continue;        // (the last lanes fetched a copy of dword TD - 1)
      uint32_t* dst = &rowbuf[wave][row & 1][0][lane + 64 * k];
      dst[0] = lo;
      dst[RS] = __builtin_amdgcn_alignbyte(hi, lo, 1);
      dst[2 * RS] = __builtin_amdgcn_alignbyte(hi, lo, 2);
      dst[3 * RS] = __builtin_amdgcn_alignbyte(hi, lo, 3);
    }
  };
  struct RowIn { uint64_t ww[NR / 2]; uint32_t ref; };
  const int rd_at = (p & 3) * RS + (p >> 2) + (DPL / 4) * q;   // this lane's first dword inside a staged row: copy p & 3, dword-aligned
  auto read_row = [&](int row, RowIn& in_) __attribute__((always_inline)) {
    const uint32_t* rb = &rowbuf[wave][row & 1][0][0] + rd_at;
#pragma unroll
    for (int k = 0; k < NR / 2; k++) in_.ww[k] = (uint64_t)rb[k] | ((uint64_t)rb[k + 1] << 32);      // each pair on its own (ds_read2_b32): one v_mqsad operand, no re-pairing
    in_.ref = (&rowbuf[wave][row & 1][0][0])[(p & 3) * RS + NRD + (p >> 2)];
  };
  if (last && has_prod && ybs - 1 >= ybsp && ybs - 1 <= ybep) load_prod(ybs - 1, g);
  uint64_t stg[NSTG];                                           // the fetch in flight: row yb + 2 at the top of row yb
  if constexpr (!VOL) {
    uint64_t d0[NSTG], d1[NSTG];
    stage_load(d0); stage_load(d1); stage_load(stg);
    stage_write(ybs, d0); stage_write(ybs + 1, d1);
  }
  // The volumes are addressed as ROW BUFFERS: a buffer resource over the row's W * D bytes (scalar registers, rebuilt per row) and one 32-bit
  // offset per lane.  Lanes outside the image have an offset outside the buffer (a negative column wraps to ~2^32): their loads return zeros
  // nobody uses and their stores are dropped — every instruction stays unconditional (the compiler can count what is in flight), no
  // clamping, and no 64-bit address arithmetic per lane (it cost ~15 vector instructions and 6 registers per row).
  // The final sweep's three stored volumes are kept as the 16-byte vectors they are loaded as: split into dwords they become separate
  // loop-carried values, the compiler gives some of them other registers at the top of the loop than the load writes, and the copy it then
  // needs waits for the load right behind it.
  constexpr int NVF = FINAL ? (WIDE ? NR / 4 : NR / 8) : 1, NVH = FINAL ? NR / 8 : 1;
  constexpr int FB = WIDE ? 2 : 1;                              // bytes per cell of the F volume
  u32x4 fF[NVF], fH0[NVH], fH1[NVH];
  auto row_rsrc = [&](const uint8_t* vol, int yb, int cell_bytes) __attribute__((always_inline)) {
    const int y = flip ? H - 1 - yb : yb;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(vol + ((size_t)frame * H + y) * W * D * cell_bytes), 0, W * D * cell_bytes, 0x00020000);
  };
  auto load_volumes = [&](int yb) __attribute__((always_inline)) {
    if constexpr (FINAL) {
      const __amdgpu_buffer_rsrc_t rF = row_rsrc(volF, yb, FB), r0 = row_rsrc(volH0, yb, 1), r1 = row_rsrc(volH1, yb, 1);
      const int off = (xl + yb) * D + 16 * q, offF = (xl + yb) * D * FB + 16 * q;
#pragma unroll
      for (int c = 0; c < NVF; c++) fF[c] = __builtin_amdgcn_raw_buffer_load_b128(rF, offF + 16 * NQ * c, 0, 0);
#pragma unroll
      for (int c = 0; c < NVH; c++) fH0[c] = __builtin_amdgcn_raw_buffer_load_b128(r0, off + 16 * NQ * c, 0, 0);
#pragma unroll
      for (int c = 0; c < NVH; c++) fH1[c] = __builtin_amdgcn_raw_buffer_load_b128(r1, off + 16 * NQ * c, 0, 0);
    }
  };
  load_volumes(ybs);
  // VOL: the lane's DPL cost bytes of its pixel, requested one row ahead into the registers the previous row's costs were just formed from.
  // The volume is indexed by the NATURAL column W-1-x_k; lanes outside the image have an offset outside the row buffer and read zeros.
  constexpr int NVC = VOL ? DPL / 16 : 1;
  u32x4 cst[NVC];
  auto load_cost = [&](int yb) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t rC = row_rsrc(cost, yb, 1);
    const int off = (W - 1 - (xl + yb)) * D + DPL * q;
#pragma unroll
    for (int c = 0; c < NVC; c++) cst[c] = __builtin_amdgcn_raw_buffer_load_b128(rC, off + 16 * c, 0, 0);
  };
  if constexpr (VOL) {
    load_cost(ybs);
#pragma unroll
    for (int c = 0; c < NVC; c++) asm volatile("" : : "v"(cst[c]));
  }
  // everything requested so far is complete before the loop starts (uses the compiler must wait for): the waits inside the loop are then
  // written for what a row leaves in flight, not for the prologue
  if constexpr (!VOL) {
#pragma unroll
    for (int k = 0; k < NSTG; k++) asm volatile("" : : "v"(stg[k]));
  }
  if constexpr (FINAL) {
#pragma unroll
    for (int k = 0; k < NVF; k++) asm volatile("" : : "v"(fF[k]));
#pragma unroll
    for (int k = 0; k < NVH; k++) asm volatile("" : : "v"(fH0[k]), "v"(fH1[k]));
  }
  // flush one row of this strip's right-image minima (minR[wave][buf]) to the row's global minima
  auto flush_minima = [&](int yb, int buf) __attribute__((always_inline)) {
    if constexpr (FINAL) {
      const int y = flip ? H - 1 - yb : yb;
      uint32_t* grow = gminR + ((size_t)frame * H + y) * W;
      uint32_t* mrow = &minR[wave][buf][0][0];
      int ln = lane;
      asm volatile("" : "+v"(ln));                              // the index arithmetic below is redone per row: hoisted out of the loop it costs a dozen registers the kernel does not have
      constexpr int KF = (NQ * MR + 63) / 64;
      uint32_t kvs[KF];
#pragma unroll
      for (int k = 0; k < KF; k++) {                            // every read first: one LDS round trip for the row instead of one per 64 entries
        const int idx = ln + 64 * k;
        kvs[k] = ((NQ * MR) % 64 == 0 || idx < NQ * MR) ? mrow[idx] : 0xFFFFFFFFu;
      }
#pragma unroll
      for (int k = 0; k < KF; k++) {
        const int idx = ln + 64 * k;
        const uint32_t kv = kvs[k];
        if (kv != 0xFFFFFFFFu) {
          mrow[idx] = 0xFFFFFFFFu;
          const int qq = idx / MR, ee = idx - qq * MR;
          const int xr = x0 + PX * wave + yb + ee + DPL * qq;
          if (xr >= 0 && xr < W) atomicMin(grow + xr, kv + (uint32_t)(DPL * qq));
        }
      }
    }
  };
  int known_p = ybs, known_c = ybs - 1;                        // cached prog[wave + 1] / cons[wave]
  // Order inside a row: everything that was loaded from memory was requested a whole row earlier, into registers that had just
  // been consumed (no second set of registers, and every wait counts only loads that are a row old):
  //   costs from the row's bytes -> request the next row's bytes;  [last strip: the producer's columns, requested a row ago]
  //   -> neighbour columns -> the three paths -> publish -> [final: S from the stored volumes -> request the next row's volumes -> winners]
  for (int yb = ybs; yb <= ybe; yb++) {
    const int y = flip ? H - 1 - yb : yb;
    const int xk = xl + yb;
    const bool in = xk >= 0 && xk < W;
    uint32_t Cp[NR], acc[NR];
    if constexpr (!VOL) {
      RowIn cur;
      read_row(yb, cur);                                       // LDS reads of the row's bytes ...
      if constexpr (FINAL) {                                   // ... in flight while the previous row's minima are flushed (their atomics were served long ago)
        __builtin_amdgcn_sched_barrier(0);
        if (yb > ybs && !SW_DBG(2)) flush_minima(yb - 1, (yb - 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      costs64<NR>(cur.ww, cur.ref & 0x00FFFFFFu, P2pk, Cp);
    } else {
      if constexpr (FINAL) {
        __builtin_amdgcn_sched_barrier(0);
        if (yb > ybs) flush_minima(yb - 1, (yb - 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      uint32_t w[NR / 2];
#pragma unroll
      for (int c = 0; c < NVC; c++) { w[4 * c] = cst[c].x; w[4 * c + 1] = cst[c].y; w[4 * c + 2] = cst[c].z; w[4 * c + 3] = cst[c].w; }
      costs_bytes<NR>(w, P2pk, Cp);
    }
#pragma unroll
    for (int r = 0; r < NR; r++) asm volatile("" : "+v"(Cp[r]) : : "memory");   // the costs are computed HERE (they would otherwise sink to their first
    __builtin_amdgcn_sched_barrier(0);                         // use, past the loads that reuse their input registers — which then get copied)
    if constexpr (VOL) load_cost(min(yb + 1, ybe));            // the next row's cost bytes
    else if (!SW_DBG(16)) { stage_write(yb + 2, stg); stage_load(stg); }   // row yb + 2 (fetched during row yb - 1) into the ring; request row yb + 3
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!FINAL) {
#pragma unroll
      for (int r = 0; r < NR; r++) acc[r] = 0u;
    }
    // ---- last strip: the producer block's columns of row yb - 1 ----
    if (last) {
      const int yr = yb - 1;
      if (has_prod && yr >= ybsp && yr <= ybep && !SW_DBG(1)) {
        // g was loaded for exactly this row (before the loop or during the previous row).  The usual case — every tag is this launch's —
        // has its own code path, so that its wait counts only what is older than g; the retry loop (the producer has not written the
        // whole row yet) reloads into other registers.
        if (__builtin_amdgcn_ballot_w64(!tags_ok(g)) == 0ull) {
          to_nextblk(g, nextblk);
        } else {
          piece_t v[NG];
          do {
            __builtin_amdgcn_s_sleep(8);
            load_prod(yr, v);
          } while (__builtin_amdgcn_ballot_w64(!tags_ok(v)) != 0ull);
          to_nextblk(v, nextblk);
        }
      } else {
#pragma unroll
        for (int k = 0; k < (SLOT + 63) / 64; k++) { const int o = lane + 64 * k; if (SLOT % 64 == 0 || o < SLOT) nextblk[o] = P2pk; }
      }
      if constexpr (!LATE_PROD) { if (has_prod && yb >= ybsp && yb <= ybep && yb < ybe && !SW_DBG(1)) load_prod(yb, g); }  // the next row's, speculatively: checked when it is needed
    }
    // ---- the right neighbour's columns of row yb - 1 ----
    const uint32_t* e;
    if (!last) {
      while (known_p < yb && !SW_DBG(32)) {
        known_p = __builtin_amdgcn_readfirstlane(lds_load_relaxed(&prog[wave + 1]));
        if (known_p < yb) __builtin_amdgcn_s_sleep(1);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
      e = &ring[(yb - 1) & (RING - 1)][wave + 1][0];
    } else {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
      e = nextblk;
    }
    // V moves one column to the left, M two (DPP row shifts; the last lanes keep their own value for the moment).  What enters from
    // the right neighbour — its column 0 of V into lane 15, its columns 0 and 1 of M into lanes 14 and 15 — is read from LDS by those
    // lanes only, straight into the shifted registers: 2 NR shifts (the first form shifted M twice: 3 NR), 8 instead of 12 LDS reads
    // and no temporaries.  The reads and the wait for them are ONE asm statement with the registers as in/out operands: the other
    // lanes keep their value (which C++ cannot say without 48 extra moves per row), and the compiler never sees the registers while
    // the reads are in flight.
    {
#pragma unroll
      for (int r = 0; r < NR; r++) {
        V[r] = (uint32_t)__builtin_amdgcn_update_dpp((int)V[r], (int)V[r], 0x101, 0xf, 0xf, false);   // row_shl:1
        M[r] = (uint32_t)__builtin_amdgcn_update_dpp((int)M[r], (int)M[r], 0x102, 0xf, 0xf, false);   // row_shl:2
      }
      u32x4 tv[NR / 4], tm[NR / 4];
#pragma unroll
      for (int k = 0; k < NR / 4; k++) { tv[k] = (u32x4){V[4 * k], V[4 * k + 1], V[4 * k + 2], V[4 * k + 3]}; tm[k] = (u32x4){M[4 * k], M[4 * k + 1], M[4 * k + 2], M[4 * k + 3]}; }
      const uint32_t aV = lds_addr(e + (0 * NQ + q) * NR), aM = lds_addr(e + ((p == PX - 2 ? 1 : 2) * NQ + q) * NR);
      lds_read_lanes<NR / 4>(tv, tm, p == PX - 1 ? aV : 0xFFFFFFFFu, p >= PX - 2 ? aM : 0xFFFFFFFFu);
#pragma unroll
      for (int k = 0; k < NR / 4; k++) {
        V[4 * k] = tv[k].x; V[4 * k + 1] = tv[k].y; V[4 * k + 2] = tv[k].z; V[4 * k + 3] = tv[k].w;
        M[4 * k] = tm[k].x; M[4 * k + 1] = tm[k].y; M[4 * k + 2] = tm[k].z; M[4 * k + 3] = tm[k].w;
      }
      if (!last) {                                             // LDS serves a wave's instructions in order: the reads above are done
        if (lane == 0) lds_store_relaxed(&cons[wave + 1], yb);
      }
    }
    if constexpr (FINAL) {
      // S starts as 8 (C + P2) - (the five stored paths) and the three upward paths subtract their Y from it.  The stored volumes — requested
      // after the previous row's paths — are consumed HERE, before the cells: their 24 registers are free while the cells hold their
      // temporaries (the kernel then fits three waves per SIMD), at the price of a shorter lead for those loads.
#pragma unroll
      for (int k = 0; k < NR / 2; k++) {
        uint32_t a, b;
        const uint32_t h0 = fH0[k >> 2][k & 3], h1 = fH1[k >> 2][k & 3];
        if constexpr (WIDE) { a = pk_add(pk_add(fF[(2 * k) >> 2][(2 * k) & 3], unpack_lo(h0)), unpack_lo(h1)); b = pk_add(pk_add(fF[(2 * k + 1) >> 2][(2 * k + 1) & 3], unpack_hi(h0)), unpack_hi(h1)); }
        else { const uint32_t hb = h0 + h1, ff = fF[k >> 2][k & 3];    // bytes <= 2 P2 <= 170: no carry between bytes
               a = pk_add(unpack_lo(ff), unpack_lo(hb)); b = pk_add(unpack_hi(ff), unpack_hi(hb)); }
        acc[2 * k] = pk_sub(pk_shl3(Cp[2 * k]), a);
        acc[2 * k + 1] = pk_sub(pk_shl3(Cp[2 * k + 1]), b);
      }
#pragma unroll
      for (int r = 0; r < NR; r++) asm volatile("" : "+v"(acc[r]));
      __builtin_amdgcn_sched_barrier(0);
    }
    {
      uint32_t upV, dnV, upG, dnG, upM, dnM, mn, Ln[NR];
      path_neighbours<NR, LQ>(V, lane, q, P1pk, upV, dnV);
      path_neighbours<NR, LQ>(G, lane, q, P1pk, upG, dnG);
      path_neighbours<NR, LQ>(M, lane, q, P1pk, upM, dnM);
      path_cells<NR, FINAL>(V, upV, dnV, Cp, acc, Ln, mn, P1pk);
      path_normalise<NR>(V, Ln, pixel_min<LQ>(mn), (uint32_t)s.P2);
      path_cells<NR, FINAL>(G, upG, dnG, Cp, acc, Ln, mn, P1pk);
      path_normalise<NR>(G, Ln, pixel_min<LQ>(mn), (uint32_t)s.P2);
      path_cells<NR, FINAL>(M, upM, dnM, Cp, acc, Ln, mn, P1pk);
      path_normalise<NR>(M, Ln, pixel_min<LQ>(mn), (uint32_t)s.P2);
    }
    if constexpr (FINAL) {
      __builtin_amdgcn_sched_barrier(0);
      if (!SW_DBG(4)) load_volumes(min(yb + 1, ybe));   // the next row's volumes: in flight during the winners, the publishing and the next row's costs
      __builtin_amdgcn_sched_barrier(0);
    }
    if (__builtin_amdgcn_ballot_w64(!in)) {                    // a strip crossing the image border: pixels outside carry Lq = 0 (a path entering the image starts with L = C)
#pragma unroll
      for (int r = 0; r < NR; r++) { V[r] = in ? V[r] : P2pk; G[r] = in ? G[r] : P2pk; M[r] = in ? M[r] : P2pk; }
    }
    if constexpr (LATE_PROD) {
      // (final sweep with eight lanes per pixel: six registers of producer columns do not fit next to the cells' temporaries — held across the
      // cells they are spilled, and a spill right behind the load is a synchronous wait.  Requested behind the cells instead, defined on every
      // path so that no old value stays alive around the loop.)
      if (last && has_prod && yb >= ybsp && yb <= ybep && yb < ybe && !SW_DBG(1)) load_prod(yb, g);
      else {
#pragma unroll
        for (int k = 0; k < NG; k++) g[k] = Px::zero();
      }
    }
    // ---- publish this strip's first two columns of row yb ----
    if (wave > 0 || j > 0) {
      if (wave > 0) {
        while (known_c < yb - RING + 1 && !SW_DBG(32)) {                      // the slot still holds row yb - RING until the left neighbour has read it
          known_c = __builtin_amdgcn_readfirstlane(lds_load_relaxed(&cons[wave]));
          if (known_c < yb - RING + 1) __builtin_amdgcn_s_sleep(1);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
      }
      uint32_t* o = &ring[yb & (RING - 1)][wave][0];
      if (p == 0) {
#pragma unroll
        for (int r = 0; r < NR; r++) { o[(0 * NQ + q) * NR + r] = V[r]; o[(1 * NQ + q) * NR + r] = M[r]; }
      }
      if (p == 1) {
#pragma unroll
        for (int r = 0; r < NR; r++) o[(2 * NQ + q) * NR + r] = M[r];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      if (wave > 0) {
        if (lane == 0) lds_store_relaxed(&prog[wave], yb + 1);
      } else {                                                 // strip 0: to the next block through memory, tagged
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
        const __amdgpu_buffer_rsrc_t rG = gx_rsrc(my_gx + (size_t)yb * SLOT);
        int ln = lane;
        asm volatile("" : "+v"(ln));
#pragma unroll
        for (int k = 0; k < NG; k++) {
          const int oo = ln + 64 * k;                           // (lanes beyond the row read a valid piece again; their store is dropped)
          const piece_t v = *reinterpret_cast<const piece_t*>(o + PW * min(oo, NP - 1)) | tagpk;
          Px::store(v, rG, 4 * PW * oo);
        }
      }
    }
    if (!last && yb < ybe) known_p = __builtin_amdgcn_readfirstlane(lds_load_relaxed(&prog[wave + 1]));   // for the next row: usually already far enough
    if constexpr (!FINAL) {
      // pixels outside the image store into the slack behind the volume: an unconditional store keeps the next row's wait for its input
      // bytes from also waiting for these stores (the compiler can then count them)
      if (!SW_DBG(4)) {
        const __amdgpu_buffer_rsrc_t rF = row_rsrc(volF, yb, FB);
        const int off = xk * D * FB + 16 * q;
        if constexpr (WIDE) {
#pragma unroll
          for (int c = 0; c < NR / 4; c++) __builtin_amdgcn_raw_buffer_store_b128((u32x4){acc[4 * c], acc[4 * c + 1], acc[4 * c + 2], acc[4 * c + 3]}, rF, off + 16 * NQ * c, 0, 0);
        } else {
#pragma unroll
          for (int c = 0; c < NR / 8; c++)
            __builtin_amdgcn_raw_buffer_store_b128((u32x4){pack4(acc[8 * c], acc[8 * c + 1]), pack4(acc[8 * c + 2], acc[8 * c + 3]), pack4(acc[8 * c + 4], acc[8 * c + 5]),
                                                           pack4(acc[8 * c + 6], acc[8 * c + 7])}, rF, off + 16 * NQ * c, 0, 0);
        }
      }
    } else {
      const uint32_t (&S)[NR] = acc;                           // S = 8 (C + P2) - (the three upward Y + the stored five)
      uint32_t key = 0xFFFFFFFFu;
      // lanes outside the image aim their minima at a trash row: the atomics are unconditional and can be issued between the instructions
      // that build the keys (32 of them back to back fill the LDS queue and stall the wave)
      uint32_t* mr = in ? &minR[wave][yb & 1][q][p] : &minR_trash[wave][q][p];
#pragma unroll
      for (int r = 0; r < NR; r++) {
        const uint32_t klo = (S[r] << 16) | (uint32_t)r, khi = (S[r] & 0xFFFF0000u) | (uint32_t)(r + NR);
        if (!SW_DBG(2)) { atomicMin(mr + r, klo); atomicMin(mr + r + NR, khi); }
        key = min(min(key, klo), khi);
      }
      key = in ? key + (uint32_t)(DPL * q) : 0xFFFFFFFFu;
      {
        if constexpr (LQ == 8) key = min(key, (uint32_t)__builtin_amdgcn_update_dpp((int)key, (int)key, 0x128, 0xf, 0xf, false));   // row_ror:8
        const auto a = __builtin_amdgcn_permlane16_swap(key, key, false, false);
        key = min(a[0], a[1]);
        const auto b = __builtin_amdgcn_permlane32_swap(key, key, false, false);
        key = min(b[0], b[1]);
      }
      const int d = (int)(key & 0xFFFFu);
      int d16 = 16 * d;
      if (s.subpixel) {
        uint32_t* my = reinterpret_cast<uint32_t*>(sS + ((size_t)(PX * wave + p) * D + DPL * q));
#pragma unroll
        for (int r = 0; r < NR; r += 2) {                      // S in disparity order: low halves are j = r, high halves j = r + NR
          my[r / 2] = __builtin_amdgcn_perm(S[r + 1], S[r], 0x05040100u);
          my[(r + NR) / 2] = __builtin_amdgcn_perm(S[r + 1], S[r], 0x07060302u);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (in && q == 0 && d > 0 && d < D - 1) {
          const uint16_t* ps = sS + (size_t)(PX * wave + p) * D;
          const int sm = ps[d - 1], sc = ps[d], sp = ps[d + 1];
          const int den = max(sm + sp - 2 * sc, 1);
          d16 = 16 * d + (16 * (sm - sp) + den) / (2 * den);
        }
      }
      // unconditional (the other lanes write into the slack behind the array): the next row's first wait can then count it
      {
        const __amdgpu_buffer_rsrc_t rD = __builtin_amdgcn_make_buffer_rsrc(dLp + ((size_t)frame * H + y) * W, 0, W * 4, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32((uint32_t)d | ((uint32_t)(uint16_t)d16 << 16), rD, q == 0 ? xk * 4 : -1, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  if constexpr (FINAL) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
    flush_minima(ybe, ybe & 1);
  }
}

