// pgx_replay_eval.hip -- the evaluation kernels of the device replay: shimmer_to_overlap (/root/reference/src/shmr_overlap.c:52-180) for the dirty
// buckets of a pass, in three shapes -- k_eval (16 lanes per bucket, the dense rounds), k_eval_rows (a wavefront per bucket, four rows per step, the
// sparse passes), k_eval_big (a workgroup per big bucket).  The fixed-point formulation and the schedule: pgx_replay.hip.
#include "pgx_replay.h"

namespace pgx {
namespace rp {

// ---- shimmer_to_overlap (shmr_overlap.c:52-180) for every dirty bucket in [lo, hi) -------------------------------------
// A group of GL lanes per bucket.  The rows (ai, descending) are sequential -- they communicate through the "contained"
// flags -- but the partners of one row are examined GL at a time, speculatively: lane l takes partner pbase + l, and the
// sequential semantics (stop once bestn overlaps are counted, or when the row's own read turns out contained) are then
// resolved with ballots.  What a lane beyond the stop did is harmless: a pair key, a reader registration (only ever costs a
// spurious re-evaluation), loads.  Buckets that hold a read twice can meet a pair twice within one evaluation: they run one
// partner at a time.  A single evaluation is a chain of dependent memory round trips, so the group form is what bounds
// the latency of a pass: rows x ~4 round trips instead of examinations x ~4.
// ---- shimmer_to_overlap (shmr_overlap.c:52-180) for every dirty bucket of the launch ------------------------------------
// A group of 16 lanes per bucket.  The rows (ai, descending) are sequential -- they communicate through the "contained"
// flags -- but the partners of one row are examined 16 at a time, speculatively: lane l takes partner pbase + l, and the
// sequential semantics (stop once bestn overlaps are counted, or when the row's own read turns out contained) are then
// resolved with ballots.  What a lane beyond the stop did is harmless: loads.  Buckets that hold a read twice can meet a
// pair twice within one evaluation: they run one partner at a time.  A single evaluation is a chain of dependent memory
// round trips, which is what bounds a sparse pass: the bucket's entries are staged in LDS once, a probe brings key and
// owner in one 16-byte load, and registrations / item stores are not waited for.
__global__ __launch_bounds__(256) void k_eval(R r, uint32_t lo, uint32_t hi, uint32_t nlist) {
  __shared__ uint32_t s_rid[GPB][128], s_pos[GPB][128], s_rl[GPB][128];
  __shared__ uint8_t s_dir[GPB][128];
  const int lane = threadIdx.x & 63, gl = lane & (GL - 1), gbase = lane & ~(GL - 1), gib = threadIdx.x / GL;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t jj = bucket_of_group(r, lo, hi, nlist, wave * GPW + (uint32_t)(lane / GL));
  const uint32_t j = (uint32_t)jj;
  bool alive = jj < hi && r.dirty[j] && !r.c->overflow;
  if (alive && (r.bflags[j] & F_BIG)) {   // a big bucket: left to k_eval_big, which runs behind this kernel from the list written here
    if (gl == 0) {
      const uint32_t at = atomicAdd(&r.c->nbig, 1u);
      if (at < LIST_CAP) r.blist[at] = j;   // (beyond the list: the bucket stays dirty and is listed again by the next pass)
    }
    alive = false;
  }
  {
    const uint64_t am = __ballot(alive);
    if (!am) return;
    if (lane == (int)__builtin_ctzll(am)) atomicAdd(&r.spread[(wave % SPREAD) * 8], (unsigned long long)(__popcll(am) / GL));
  }
  // reader-node arena: wave-uniform cursor; the wavefront that evaluates these buckets next time continues where this one stops
  const uint32_t wave_id = nlist ? r.wlist0 + wave : (uint32_t)(((uint64_t)lo + (uint64_t)wave * GPW) / GPW);
  const uint4 wc = r.wcur[wave_id];
  uint32_t rcur = wc.x, rend = wc.y;
  uint32_t icur = wc.z, iend = wc.w;   // item arena of this wavefront slot (multiples of 16), same idea
  uint32_t s0 = 0, n = 0;
  bool dup = false, first_eval = true;
  if (alive) {
    const uint32_t b = r.bid[j];
    s0 = r.bstart[b], n = r.bstart[b + 1] - s0;
    dup = (r.bflags[j] & F_DUP) != 0;
    first_eval = r.ever[j] == 0;
    for (uint32_t i = (uint32_t)gl; i < n; i += GL) {  // the bucket's entries -> LDS
      const uint64_t y = r.y0[s0 + i];
      const uint32_t rid = (uint32_t)(y >> 32);
      s_rid[gib][i] = rid, s_pos[gib][i] = (((uint32_t)y) >> 1) + 1, s_dir[gib][i] = r.dir[s0 + i], s_rl[gib][i] = r.rlen[rid];
    }
    if (gl == 0) {
      r.dirty[j] = 0;
      r.evaluated[j] = 1;
      r.ever[j] = 1;
      r.parity[j] ^= 1;
      r.ohead[j] = r.ihead[j];
    }
  }
  uint64_t clo = 0, chi = 0;  // "contained" flags of the bucket's entries (n <= 128)
  auto cget = [&](uint32_t i) { return (((i < 64 ? clo : chi) >> (i & 63)) & 1) != 0; };
  uint32_t head = NIL, num = 0, lookups = 0, skips = 0;
  uint32_t chunk = 0;  // base of the item chunk holding insertion ordinals [num & ~15, ...)
  bool any_guess = false, any_unfiled = false;
  int ai = (int)n - 1;  // (the first row opened is n - 2)
  bool row_open = false;
  uint32_t pbase = 0, got = 0, rid0 = 0, pos0 = 0, rlen0 = 0, dir0 = 0;
  bool p_reg = false;  // this lane has a registration whose list position (p_idx) has not been looked at yet
  uint32_t p_idx = 0, p_slot = 0;
  auto resolve_pending = [&]() -> bool {  // false: the reader-node arena is exhausted
    if (p_reg && p_idx < NIN) r.pc[p_slot >> r.cshift].in[p_idx] = j + 1, p_reg = false;
    const uint64_t rm = __ballot(p_reg);  // (what is left goes to the linked overflow)
    if (rm) {
      const uint32_t total = (uint32_t)__popcll(rm);
      if (rcur + total > rend) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&r.c->rnode_top, NCH);
        base = (uint32_t)__shfl((int)base, 0, 64);
        if ((uint64_t)base + NCH > r.rn_cap) {
          atomicOr(&r.c->overflow, OV_NODES);
          return false;
        }
        rcur = base, rend = base + NCH;
      }
      if (p_reg) {
        const uint32_t node = rcur + lane_rank(rm);
        const uint32_t old = atomicExch(&r.pc[p_slot >> r.cshift].rhead, node + 1);
        r.rn[node] = RNode{old, j};
      }
      rcur += total;
      p_reg = false;
    }
    return true;
  };
  for (;;) {
    if (alive && !row_open) {
      do --ai;
      while (ai >= 0 && cget((uint32_t)ai));
      if (ai < 0 || r.bestn == 0) {  // the bucket is done
        if (gl == 0) {
          r.ihead[j] = head, r.inum[j] = num, r.lookups[j] = lookups, r.skips[j] = skips;
          r.bflags[j] = (uint8_t)((dup ? F_DUP : 0) | (any_guess ? F_GUESS : 0) | (any_unfiled ? F_UNFILED : 0));
        }
        alive = false;
      } else {
        rid0 = s_rid[gib][ai], pos0 = s_pos[gib][ai], rlen0 = s_rl[gib][ai], dir0 = s_dir[gib][ai];
        got = 0, pbase = (uint32_t)ai + 1, row_open = true;
      }
    }
    if (!__ballot(alive)) {
      if (!resolve_pending()) return;
      if (lane == 0) r.wcur[wave_id] = make_uint4(rcur, rend, icur, iend);
      break;
    }
    // ---- one batch of partners ----
    const uint32_t step = dup ? 1u : (uint32_t)GL;
    const uint32_t pi = pbase + (uint32_t)gl;
    bool valid = alive && (uint32_t)gl < step && pi < n && !cget(pi);
    uint32_t rid1 = 0, pos1 = 0;
    if (valid) {
      rid1 = s_rid[gib][pi], pos1 = s_pos[gib][pi];
      if (rid1 == rid0) valid = false;
    }
    uint32_t slot = NONE, v = 0;
    const uint64_t pair = rid0 < rid1 ? ((uint64_t)rid0 << 32 | rid1) : ((uint64_t)rid1 << 32 | rid0);
    if (valid) slot = pair_find(r, pair, &v);
    const uint64_t vm = __ballot(valid);
    bool present = false, accepted = false, guessed = false;
    uint32_t ptype = 0, type = 0, mslot = NONE;
    if (valid) {
      present = v != 0 && own_bucket(v) < j;
      ptype = present ? own_type(v) : 0;
      if (!present && dup && slot != NONE)  // inserted earlier in THIS evaluation?
        for (uint32_t it = head; it != NIL; it = r.items[it - 1].next)
          if (r.items[it - 1].pslot == slot) {
            present = true, ptype = (r.items[it - 1].info >> 16) & 3;
            break;
          }
      if (!present) {
        const uint32_t rlen1 = s_rl[gib][pi], dir1 = s_dir[gib][pi];
        const uint32_t q_off = pos0 - pos1;
        if (q_off >= (1u << 30)) atomicOr(&r.c->overflow, OV_QOFF);
        uint32_t req = NONE;
        if (r.memo_used) mslot = memo_find(r, (unsigned long long)rid0 << 32 | rid1, q_off << 2 | dir0 << 1 | dir1, &req);
        if (req < r.settled) {
          accepted = classify(r.rq_res[req], rlen0, rlen1, q_off, &type);
        } else {
          accepted = true, guessed = true, type = T_OVERLAP;
          if (r.predict && predict_contained(rlen0, rlen1, q_off, r.predict, r.predict2)) type = rlen0 >= rlen1 ? T_CONTAINS : T_CONTAINED;
        }
      }
    }
    if (!resolve_pending()) return;  // (the previous batch's registrations: their atomics have returned behind the loads above)
    // ---- the sequential semantics of the row over this batch, lowest partner first ----
    const uint64_t Vg = gbits(vm, gbase);
    const uint64_t P = gbits(__ballot(valid && present), gbase);
    const uint64_t PO = gbits(__ballot(valid && present && ptype == T_OVERLAP), gbase);
    const uint64_t A = gbits(__ballot(valid && !present && accepted), gbase);
    const uint64_t AO = gbits(__ballot(valid && !present && accepted && type == T_OVERLAP), gbase);
    const uint64_t AC = gbits(__ballot(valid && !present && accepted && type == T_CONTAINED), gbase);
    uint64_t AP = gbits(__ballot(valid && !present && accepted && type == T_CONTAINS), gbase);
    const uint64_t inc = PO | AO;
    int stop = GL;  // the last partner the sequential loop processes in this batch (GL: all of them, and the row goes on)
    if (alive && row_open) {
      const uint32_t need = r.bestn - got;  // >= 1
      if ((uint32_t)__popcll(inc) >= need) {
        uint64_t m = inc;
        for (uint32_t k = 1; k < need; ++k) m &= m - 1;
        stop = __builtin_ctzll(m);
      }
      if (AC) stop = min(stop, (int)__builtin_ctzll(AC));
    }
    const uint64_t proc = (2ULL << stop) - 1ULL;
    const uint64_t ins = A & proc;
    {  // the partners the sequential loop really examined register as readers of their pairs (the lists are only read by
       // k_update, after this kernel); a bucket listed by an earlier evaluation is not listed again.  The list position comes
       // from an atomic whose result is only looked at after the NEXT batch's loads have been issued (resolve_pending).
      bool reg = valid && ((proc >> gl) & 1);
      if (reg && slot == NONE) slot = pair_slot(r, pair);  // a pair the walk really examines gets its slot now
      if (reg && !first_eval) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(&r.pc[slot >> r.cshift]);
        const uint4 h1 = *reinterpret_cast<const uint4 *>(w);  // cnt, rhead, in[0], in[1]
        const uint32_t c = min(h1.x, NIN);
        if ((c > 0 && h1.z == j + 1) || (c > 1 && h1.w == j + 1)) reg = false;
        for (uint32_t q = 2; q < c && reg; q += 8) {
          const uint4 a = *reinterpret_cast<const uint4 *>(w + 2 + q), b = *reinterpret_cast<const uint4 *>(w + 6 + q);
          const uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
          for (uint32_t k = 0; k < 8; ++k)
            if (q + k < c && x[k] == j + 1) reg = false;
        }
      }
      if (reg) p_idx = atomicAdd(&r.pc[slot >> r.cshift].cnt, 1u), p_slot = slot, p_reg = true;
    }
    // ---- the batch's insertions: the bucket's items fill 16-aligned chunks of 16 in insertion order (k_update walks a
    // bucket's list a chunk at a time, one lane per item) ----
    const bool my_ins = valid && !present && accepted && ((proc >> gl) & 1);
    const uint32_t cins = (uint32_t)__popcll(ins);
    const bool need_chunk = cins != 0 && (num == 0 || ((num + cins - 1) >> 4) != ((num - 1) >> 4));  // group-uniform
    uint32_t fresh = 0;
    {
      const uint64_t cm = __ballot(need_chunk && gl == 0);
      if (cm) {
        const uint32_t want = 16u * (uint32_t)__popcll(cm);
        if (icur + want > iend) {  // refill: one atomic on the shared counter per ICH items instead of one per chunk
          const uint32_t take = want > ICH ? want : ICH;
          uint32_t base = 0;
          if (lane == (int)__builtin_ctzll(cm)) base = atomicAdd(&r.c->item_top, take);
          base = (uint32_t)__shfl((int)base, (int)__builtin_ctzll(cm), 64);
          if ((uint64_t)base + take > r.item_cap) {
            atomicOr(&r.c->overflow, OV_ITEMS);
            return;
          }
          icur = base, iend = base + take;   // (what was left of the old piece, < want, is not used)
        }
        fresh = icur + 16u * (uint32_t)__popcll(cm & ((1ULL << gbase) - 1ULL));  // (gl == 0 lanes: one bit per group)
        icur += want;
      }
    }
    if (cins) {
      if (my_ins) {
        const uint32_t ord = num + (uint32_t)__popcll(ins & ((1ULL << gl) - 1ULL));  // insertion ordinal within the bucket
        const bool in_fresh = need_chunk && (num == 0 || (ord >> 4) != ((num - 1) >> 4));
        const uint32_t idx = (in_fresh ? fresh : chunk) + (ord & 15);
        uint32_t next;
        if (ord == 0) next = NIL;
        else if ((ord & 15) == 0) next = chunk + 16;  // the last item of the previous chunk, + 1
        else next = idx;                              // the item before this one, + 1
        uint32_t info = (uint32_t)ai | pi << 8 | type << 16;
        if (guessed) info |= I_GUESS;
        if (mslot == NONE) info |= I_UNFILED;
        r.items[idx] = Item{slot, info, mslot, next};
      }
      const uint32_t last = num + cins - 1;
      if (need_chunk && (num == 0 || (last >> 4) != ((num - 1) >> 4))) chunk = fresh;
      head = chunk + (last & 15) + 1;
      num += cins;
    }
    {
      const uint64_t g1 = gbits(__ballot(my_ins && guessed), gbase), g2 = gbits(__ballot(my_ins && mslot == NONE), gbase);
      any_guess |= g1 != 0, any_unfiled |= g2 != 0;
    }
    if (alive && row_open) {
      got += (uint32_t)__popcll(inc & proc);
      skips += (uint32_t)__popcll(P & proc);
      lookups += (uint32_t)__popcll(Vg & ~P & proc);
      AP &= proc;
      if (AP) {  // partners found contained: entry pbase + l
        if (pbase < 64) {
          clo |= AP << pbase;
          if (pbase) chi |= AP >> (64 - pbase);
        } else {
          chi |= AP << (pbase - 64);
        }
      }
      if (AC & proc) {
        if (ai < 64) clo |= 1ULL << ai;
        else chi |= 1ULL << (ai - 64);
      }
      if (stop < GL || pbase + step >= n) row_open = false;
      else pbase += step;
    }
  }
}

// ---- the same evaluation with FOUR ROWS PER STEP, for the sparse passes (a wavefront per bucket: lanes are plentiful there and
// a pass lasts as long as its longest bucket's chain of rows).  Lane l works row l / PW, partner l % PW; the rows are committed
// in order while each one is complete within its PW partners and no earlier row of the step set a contained flag (then the
// rows below are looked at again with the new flags); a row that needs more partners is continued alone, GLT per step.
template <int GLT, int PW>
__global__ __launch_bounds__(256) void k_eval_rows(R r, uint32_t lo, uint32_t hi, uint32_t nlist) {
  constexpr uint32_t GPWT = 64 / GLT, GPBT = 256 / GLT;
  constexpr int SH = PW == 16 ? 4 : 2;  // log2(PW)
  constexpr uint64_t RM = (1ULL << PW) - 1ULL;  // one row's lanes
  __shared__ uint32_t s_rid[GPBT][128], s_pos[GPBT][128], s_rl[GPBT][128];
  __shared__ uint8_t s_dir[GPBT][128];
  const int lane = threadIdx.x & 63, gl = lane & (GLT - 1), gbase = lane & ~(GLT - 1), gib = threadIdx.x / GLT;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t jj = bucket_of_group(r, lo, hi, nlist, wave * GPWT + (uint32_t)(lane / GLT));
  const uint32_t j = (uint32_t)jj;
  bool alive = jj < hi && r.dirty[j] && !r.c->overflow;
  if (alive && (r.bflags[j] & F_BIG)) {   // a big bucket: left to k_eval_big, which runs behind this kernel from the list written here
    if (gl == 0) {
      const uint32_t at = atomicAdd(&r.c->nbig, 1u);
      if (at < LIST_CAP) r.blist[at] = j;   // (beyond the list: the bucket stays dirty and is listed again by the next pass)
    }
    alive = false;
  }
  {
    const uint64_t am = __ballot(alive);
    if (!am) return;
    if (lane == (int)__builtin_ctzll(am)) atomicAdd(&r.spread[(wave % SPREAD) * 8], (unsigned long long)(__popcll(am) / GLT));
  }
  // reader-node arena: wave-uniform cursor; the wavefront that evaluates these buckets next time continues where this one stops
  const uint32_t wave_id = nlist ? r.wlist0 + wave : (uint32_t)(((uint64_t)lo + (uint64_t)wave * GPWT) / GPWT);
  const uint4 wc = r.wcur[wave_id];
  uint32_t rcur = wc.x, rend = wc.y;
  uint32_t icur = wc.z, iend = wc.w;   // item arena of this wavefront slot (multiples of 16), same idea
  uint32_t s0 = 0, n = 0;
  bool dup = false, first_eval = true;
  if (alive) {
    const uint32_t b = r.bid[j];
    s0 = r.bstart[b], n = r.bstart[b + 1] - s0;
    dup = (r.bflags[j] & F_DUP) != 0;
    first_eval = r.ever[j] == 0;
    for (uint32_t i = (uint32_t)gl; i < n; i += GLT) {  // the bucket's entries -> LDS
      const uint64_t y = r.y0[s0 + i];
      const uint32_t rid = (uint32_t)(y >> 32);
      s_rid[gib][i] = rid, s_pos[gib][i] = (((uint32_t)y) >> 1) + 1, s_dir[gib][i] = r.dir[s0 + i], s_rl[gib][i] = r.rlen[rid];
    }
    if (gl == 0) {
      r.dirty[j] = 0;
      r.evaluated[j] = 1;
      r.ever[j] = 1;
      r.parity[j] ^= 1;
      r.ohead[j] = r.ihead[j];
    }
  }
  auto gbits = [&](uint64_t wave_mask, int) { return GLT == 64 ? wave_mask : ((wave_mask >> gbase) & ((1ULL << (GLT & 63)) - 1ULL)); };
  uint64_t clo = 0, chi = 0;  // "contained" flags of the bucket's entries (n <= 128)
  auto cget = [&](uint32_t i) { return (((i < 64 ? clo : chi) >> (i & 63)) & 1) != 0; };
  auto cset = [&](uint32_t i) {
    if (i < 64) clo |= 1ULL << i;
    else chi |= 1ULL << (i - 64);
  };
  uint32_t head = NIL, num = 0, lookups = 0, skips = 0;
  uint32_t chunk = 0;  // base of the item chunk holding insertion ordinals [num & ~15, ...)
  bool any_guess = false, any_unfiled = false;
  int done_to = (int)n - 1;  // rows >= done_to are finished (the first row is n - 2)
  bool row_open = false;     // a single row (cur_row) is in progress, sixteen partners per step from pbase
  int cur_row = 0, a0 = -1, a1 = -1, a2 = -1, a3 = -1, nrows = 0;
  uint32_t pbase = 0, got = 0;
  bool p_reg = false;  // this lane has a registration whose list position (p_idx) has not been looked at yet
  uint32_t p_idx = 0, p_slot = 0;
  auto resolve_pending = [&]() -> bool {  // false: the reader-node arena is exhausted
    if (p_reg && p_idx < NIN) r.pc[p_slot >> r.cshift].in[p_idx] = j + 1, p_reg = false;
    const uint64_t rm = __ballot(p_reg);  // (what is left goes to the linked overflow)
    if (rm) {
      const uint32_t total = (uint32_t)__popcll(rm);
      if (rcur + total > rend) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&r.c->rnode_top, NCH);
        base = (uint32_t)__shfl((int)base, 0, 64);
        if ((uint64_t)base + NCH > r.rn_cap) {
          atomicOr(&r.c->overflow, OV_NODES);
          return false;
        }
        rcur = base, rend = base + NCH;
      }
      if (p_reg) {
        const uint32_t node = rcur + lane_rank(rm);
        const uint32_t old = atomicExch(&r.pc[p_slot >> r.cshift].rhead, node + 1);
        r.rn[node] = RNode{old, j};
      }
      rcur += total;
      p_reg = false;
    }
    return true;
  };
  for (;;) {
    if (alive && !row_open) {  // the next (up to four) rows that are not contained
      nrows = 0, a0 = a1 = a2 = a3 = -1;
      int x = done_to;
      while (nrows < 4) {
        do --x;
        while (x >= 0 && cget((uint32_t)x));
        if (x < 0) break;
        if (nrows == 0) a0 = x;
        else if (nrows == 1) a1 = x;
        else if (nrows == 2) a2 = x;
        else a3 = x;
        ++nrows;
      }
      if (nrows == 0 || r.bestn == 0) {  // the bucket is done
        if (gl == 0) {
          r.ihead[j] = head, r.inum[j] = num, r.lookups[j] = lookups, r.skips[j] = skips;
          r.bflags[j] = (uint8_t)((dup ? F_DUP : 0) | (any_guess ? F_GUESS : 0) | (any_unfiled ? F_UNFILED : 0));
        }
        alive = false;
      } else if (dup) {
        cur_row = a0, got = 0, pbase = (uint32_t)a0 + 1, row_open = true;
      }
    }
    if (!__ballot(alive)) {
      if (!resolve_pending()) return;
      if (lane == 0) r.wcur[wave_id] = make_uint4(rcur, rend, icur, iend);
      break;
    }
    // ---- this step's (row, partner) of the lane ----
    const bool single = row_open;  // group-uniform
    const uint32_t step = dup ? 1u : (uint32_t)GLT;
    const int q = gl >> SH;
    const int myrow = single ? cur_row : (q == 0 ? a0 : q == 1 ? a1 : q == 2 ? a2 : a3);
    const uint32_t pi = single ? pbase + (uint32_t)gl : (uint32_t)(myrow + 1 + (gl & (PW - 1)));
    bool valid = alive && (single ? (uint32_t)gl < step : q < nrows) && pi < n && !cget(pi);
    uint32_t rid0 = 0, pos0 = 0, rlen0 = 0, dir0 = 0, rid1 = 0, pos1 = 0;
    if (valid) {
      rid0 = s_rid[gib][myrow], pos0 = s_pos[gib][myrow], rlen0 = s_rl[gib][myrow], dir0 = s_dir[gib][myrow];
      rid1 = s_rid[gib][pi], pos1 = s_pos[gib][pi];
      if (rid1 == rid0) valid = false;
    }
    uint32_t slot = NONE, v = 0;
    const uint64_t pair = rid0 < rid1 ? ((uint64_t)rid0 << 32 | rid1) : ((uint64_t)rid1 << 32 | rid0);
    if (valid) slot = pair_find(r, pair, &v);
    const uint64_t vm = __ballot(valid);
    bool present = false, accepted = false, guessed = false;
    uint32_t ptype = 0, type = 0, mslot = NONE;
    if (valid) {
      present = v != 0 && own_bucket(v) < j;
      ptype = present ? own_type(v) : 0;
      if (!present && dup && slot != NONE)  // inserted earlier in THIS evaluation?
        for (uint32_t it = head; it != NIL; it = r.items[it - 1].next)
          if (r.items[it - 1].pslot == slot) {
            present = true, ptype = (r.items[it - 1].info >> 16) & 3;
            break;
          }
      if (!present) {
        const uint32_t rlen1 = s_rl[gib][pi], dir1 = s_dir[gib][pi];
        const uint32_t q_off = pos0 - pos1;
        if (q_off >= (1u << 30)) atomicOr(&r.c->overflow, OV_QOFF);
        uint32_t req = NONE;
        if (r.memo_used) mslot = memo_find(r, (unsigned long long)rid0 << 32 | rid1, q_off << 2 | dir0 << 1 | dir1, &req);
        if (req < r.settled) {
          accepted = classify(r.rq_res[req], rlen0, rlen1, q_off, &type);
        } else {
          accepted = true, guessed = true, type = T_OVERLAP;
          if (r.predict && predict_contained(rlen0, rlen1, q_off, r.predict, r.predict2)) type = rlen0 >= rlen1 ? T_CONTAINS : T_CONTAINED;
        }
      }
    }
    if (!resolve_pending()) return;  // (the previous step's registrations: their atomics have returned behind the loads above)
    // ---- the sequential semantics over this step, lowest lane first ----
    const uint64_t Vg = gbits(vm, gbase);
    const uint64_t P = gbits(__ballot(valid && present), gbase);
    const uint64_t PO = gbits(__ballot(valid && present && ptype == T_OVERLAP), gbase);
    const uint64_t A = gbits(__ballot(valid && !present && accepted), gbase);
    const uint64_t AO = gbits(__ballot(valid && !present && accepted && type == T_OVERLAP), gbase);
    const uint64_t AC = gbits(__ballot(valid && !present && accepted && type == T_CONTAINED), gbase);
    const uint64_t AP = gbits(__ballot(valid && !present && accepted && type == T_CONTAINS), gbase);
    const uint64_t inc = PO | AO;
    uint64_t proc = 0;  // the lanes the sequential walk really visits in this step
    if (alive && single) {
      int stop = GLT;  // the last partner the row processes in this step (GLT: all of them, and the row goes on)
      const uint32_t need = r.bestn - got;  // >= 1
      if ((uint32_t)__popcll(inc) >= need) {
        uint64_t m = inc;
        for (uint32_t k = 1; k < need; ++k) m &= m - 1;
        stop = __builtin_ctzll(m);
      }
      if (AC) stop = min(stop, (int)__builtin_ctzll(AC));
      proc = stop >= 63 ? ~0ULL : ((2ULL << stop) - 1ULL);
      got += (uint32_t)__popcll(inc & proc);
      for (uint64_t m = AP & proc; m; m &= m - 1) cset(pbase + (uint32_t)__builtin_ctzll(m));  // partners found contained
      if (AC & proc) cset((uint32_t)cur_row);
      if (stop < GLT || pbase + step >= n) row_open = false, done_to = cur_row;
      else pbase += step;
    } else if (alive) {
      int committed = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k >= nrows || committed != k) continue;
        const int row = k == 0 ? a0 : k == 1 ? a1 : k == 2 ? a2 : a3;
        // partners an EARLIER row of this step found contained (or that were such a row) are not examined by this row: their lanes are
        // dropped from its masks here (round 3 ended the step at the first row that changed a flag; a row's partners lie above it, so
        // the rows themselves are never flagged by an earlier row of the step)
        const uint32_t gone = (uint32_t)shr128(M128{clo, chi}, (uint32_t)row + 1).lo & (uint32_t)RM;
        const uint32_t inc_k = (uint32_t)((inc >> (PW * k)) & RM) & ~gone, ac_k = (uint32_t)((AC >> (PW * k)) & RM) & ~gone,
                       ap_k = (uint32_t)((AP >> (PW * k)) & RM) & ~gone;
        int stop = PW;
        if ((uint32_t)__popc(inc_k) >= r.bestn) {
          uint32_t m = inc_k;
          for (uint32_t t = 1; t < r.bestn; ++t) m &= m - 1;
          stop = __builtin_ctz(m);
        }
        if (ac_k) stop = min(stop, (int)__builtin_ctz(ac_k));
        if (stop == PW && (uint32_t)row + 1 + PW < n) continue;  // the row needs more partners: it is continued alone (committed stays k)
        const uint32_t proc_k = (stop < PW ? (2u << stop) - 1u : (uint32_t)RM) & ~gone;
        proc |= (uint64_t)proc_k << (PW * k);
        ++committed;
        for (uint32_t m = ap_k & proc_k; m; m &= m - 1) cset((uint32_t)row + 1 + (uint32_t)__builtin_ctz(m));   // partners found contained
        if (ac_k & proc_k) cset((uint32_t)row);
      }
      if (committed == 0) cur_row = a0, got = 0, pbase = (uint32_t)a0 + 1, row_open = true;  // (nothing done in this step)
      else done_to = committed == 1 ? a0 : committed == 2 ? a1 : committed == 3 ? a2 : a3;
    }
    skips += (uint32_t)__popcll(P & proc);
    lookups += (uint32_t)__popcll(Vg & ~P & proc);
    const uint64_t ins = A & proc;
    {  // the partners the walk really examined register as readers of their pairs (the lists are only read by k_update, after
       // this kernel); a bucket listed by an earlier evaluation is not listed again.  The list position comes from an atomic
       // whose result is only looked at after the NEXT step's loads have been issued (resolve_pending).
      bool reg = valid && ((proc >> gl) & 1);
      if (reg && slot == NONE) slot = pair_slot(r, pair);  // a pair the walk really examines gets its slot now
      if (reg && !first_eval) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(&r.pc[slot >> r.cshift]);
        const uint4 h1 = *reinterpret_cast<const uint4 *>(w);  // cnt, rhead, in[0], in[1]
        const uint32_t c = min(h1.x, NIN);
        if ((c > 0 && h1.z == j + 1) || (c > 1 && h1.w == j + 1)) reg = false;
        for (uint32_t qq = 2; qq < c && reg; qq += 8) {
          const uint4 a = *reinterpret_cast<const uint4 *>(w + 2 + qq), b = *reinterpret_cast<const uint4 *>(w + 6 + qq);
          const uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
          for (uint32_t k = 0; k < 8; ++k)
            if (qq + k < c && x[k] == j + 1) reg = false;
        }
      }
      if (reg) p_idx = atomicAdd(&r.pc[slot >> r.cshift].cnt, 1u), p_slot = slot, p_reg = true;
    }
    // ---- the step's insertions: the bucket's items fill 16-aligned chunks of 16 in insertion order (lane order is the
    // sequential order; k_update walks a bucket's list a chunk at a time, one lane per item) ----
    const bool my_ins = valid && !present && accepted && ((proc >> gl) & 1);
    const uint32_t cins = (uint32_t)__popcll(ins);  // up to 64 in one step here: it may open several 16-item chunks
    static_assert(GLT == 64, "one bucket per wavefront: the chunk allocation below is wave-uniform");
    if (cins) {
      const uint32_t cur_no = num ? (num - 1) >> 4 : 0;                 // number of the chunk `chunk` (meaningless while num == 0)
      const uint32_t first_new = num ? cur_no + 1 : 0;                   // number of the first chunk this step has to open
      const uint32_t last = num + cins - 1, last_no = last >> 4;
      const uint32_t nnew = last_no + 1 > first_new ? last_no + 1 - first_new : 0;
      uint32_t fresh = 0;
      if (nnew) {
        const uint32_t want = 16u * nnew;
        if (icur + want > iend) {
          const uint32_t take = want > ICH ? want : ICH;
          uint32_t base = 0;
          if (lane == 0) base = atomicAdd(&r.c->item_top, take);
          base = (uint32_t)__shfl((int)base, 0, 64);
          if ((uint64_t)base + take > r.item_cap) {
            atomicOr(&r.c->overflow, OV_ITEMS);
            return;
          }
          icur = base, iend = base + take;
        }
        fresh = icur, icur += want;
      }
      auto base_of = [&](uint32_t no) { return no >= first_new ? fresh + 16u * (no - first_new) : chunk; };
      if (my_ins) {
        const uint32_t ord = num + (uint32_t)__popcll(ins & ((1ULL << gl) - 1ULL));  // insertion ordinal within the bucket
        const uint32_t idx = base_of(ord >> 4) + (ord & 15);
        uint32_t next;
        if (ord == 0) next = NIL;
        else if ((ord & 15) == 0) next = base_of((ord >> 4) - 1) + 16;  // the last item of the previous chunk, + 1
        else next = idx;                                                // the item before this one, + 1
        uint32_t info = (uint32_t)myrow | pi << 8 | type << 16;
        if (guessed) info |= I_GUESS;
        if (mslot == NONE) info |= I_UNFILED;
        r.items[idx] = Item{slot, info, mslot, next};
      }
      chunk = base_of(last_no);
      head = chunk + (last & 15) + 1;
      num += cins;
    }
    {
      const uint64_t g1 = gbits(__ballot(my_ins && guessed), gbase), g2 = gbits(__ballot(my_ins && mslot == NONE), gbase);
      any_guess |= g1 != 0, any_unfiled |= g2 != 0;
    }
  }
}
template __global__ void k_eval_rows<64, 16>(R r, uint32_t lo, uint32_t hi, uint32_t nlist);

// ---- the same evaluation by a WHOLE WORKGROUP, in three phases (pgx_replay.h: LOOK / WALK / COMMIT) -------------------------------------
// LOOK: every (row, partner) pair of the bucket is looked up once -- pair table, memo, settled result or guess -- LOOK_NB pairs per lane at a
// time, the probes of all of them issued before any is tested; what the walk needs of a pair is one byte in LDS.  Nothing the lookups read
// changes while the evaluation kernels run (owners: k_update; memo: k_file; results: the alignment launches; `settled`: the host).
// WALK: wavefront 0 alone, on LDS alone and without a barrier: a row at a time, 64 partners per pass, the pass's ballots in scalar registers and
// the row's stop and cut scalar arithmetic; what it visits and inserts is noted in two masks per row.  The other wavefronts wait in front of COMMIT.
// COMMIT: the visited pairs register as readers, the inserted ones become the bucket's item list, in walk order (row, then partner).
// The walk's one exchange between lanes (the pair set of a bucket that holds a read twice: a pass's insertions are probed by the next) goes through
// LDS within ONE wavefront, whose LDS instructions execute in program order: all it needs is that the compiler keeps that order (as PH_SYNC in
// pgx_align.hip).  What a pass costs and where the time of a launch goes: profiles/eval_big_walk.txt.
#define BIG_WAVE_SYNC() __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"), __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront")
__global__ __launch_bounds__(64 * BIG_NW) void k_eval_big(R r, uint32_t lo, uint32_t hi, uint32_t nlist) {
  __shared__ uint32_t s_rid[128], s_pos[128], s_rl[128];
  __shared__ uint8_t s_dir[128];
  __shared__ uint32_t s_fresh, s_abort, s_bail;
  __shared__ uint32_t s_walk[4];                      // what the walk hands to COMMIT and the final write: num, lookups, skips, any_guess | any_unfiled << 1
  __shared__ unsigned long long s_setk[SET_CAP];      // pairs inserted by this evaluation (key + 1; 0: empty) ...
  __shared__ uint8_t s_sett[SET_CAP];                 // ... and their types
  __shared__ uint16_t s_same[128];                    // dup buckets, per entry: the nearest EARLIER entry of the same read (+ 1; 0: none) | 0x100: the read stands in the bucket more than once
  __shared__ uint8_t s_fact[128 * 128];               // LOOK's byte per pair, [row][partner] (FACT_*)
  __shared__ M128 s_vis[128], s_ins[128];             // per row: the partners (bit = entry index) the walk visited / inserted
  __shared__ uint32_t s_rbase[128], s_wsum[2];        // insertion ordinal of a row's first insertion; the scan's per-wavefront sums
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t wave_id = r.wbig0 + blockIdx.x * BIG_NW + (uint32_t)w;
  const uint4 wc = r.wcur[wave_id];
  uint32_t rcur = wc.x, rend = wc.y;   // reader-node arena of this wavefront
  uint32_t icur = wc.z, iend = wc.w;   // item arena of the workgroup (only thread 0's copy is used)
  if (threadIdx.x == 0) s_abort = 0;
  // its buckets: the big list of the pass.  Two kinds of entries: a bucket id, noted by a narrow kernel that ran over a RANGE and met the
  // bucket (k_eval / k_eval_rows skip big buckets); and a position in the dirty list | 2^31, noted by the count that made the list
  // (k_count_b) -- those count only in a list-mode launch, and only below `lo` = the number of list entries the narrow kernel and the
  // k_update of this pass cover (an evaluation k_update does not see would be lost)
  const uint32_t list_limit = nlist ? lo : 0u;
  const uint32_t nbig = min(r.c->nbig, LIST_CAP);
  for (uint32_t g = blockIdx.x; g < nbig; g += gridDim.x) {
  {
    const uint32_t e = r.blist[g];
    if ((e & 0x80000000u) && (e & 0x7FFFFFFFu) >= list_limit) continue;   // (workgroup-uniform)
    const uint32_t j = (e & 0x80000000u) ? (r.dlist[e & 0x7FFFFFFFu] & 0x7FFFFFFFu) : e;
    __syncthreads();   // (the previous bucket's LDS is done with)
    if (threadIdx.x == 0) {   // one thread decides for the workgroup (a flag another workgroup raises meanwhile must not split it)
      if (r.c->overflow) s_abort = 1;
      s_bail = 0, s_fresh = (j < hi && r.dirty[j]) ? 1u : 0u;   // (s_fresh doubles as "go": a listed bucket is dirty unless the list is stale)
    }
    __syncthreads();
    if (s_abort) break;
    if (!s_fresh) continue;
    const uint32_t b = r.bid[j], s0 = r.bstart[b], n = r.bstart[b + 1] - s0;
    const bool first_eval = r.ever[j] == 0;
    const bool dup = (r.bflags[j] & F_DUP) != 0;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      const uint64_t y = r.y0[s0 + i];
      const uint32_t rid = (uint32_t)(y >> 32);
      s_rid[i] = rid, s_pos[i] = (((uint32_t)y) >> 1) + 1, s_dir[i] = r.dir[s0 + i], s_rl[i] = r.rlen[rid];
    }
    if (threadIdx.x < 128) s_vis[threadIdx.x] = M128{0, 0}, s_ins[threadIdx.x] = M128{0, 0};
    if (dup) {
      for (uint32_t i = threadIdx.x; i < SET_CAP; i += blockDim.x) s_setk[i] = 0;
    }
    __syncthreads();   // (entries staged; everybody has read ever[] / dirty[] / bflags[] before thread 0 changes them)
    if (dup) {   // which entries share their read with another one (only pairs with such an entry can be met twice in one evaluation)
      for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t me = s_rid[i];
        uint32_t prev = 0, more = 0;
        for (uint32_t k = 0; k < n; ++k) {
          const bool same = s_rid[k] == me && k != i;
          more |= same ? 0x100u : 0u;
          if (same && k < i) prev = k + 1;
        }
        s_same[i] = (uint16_t)(prev | more);
      }
    }
    if (threadIdx.x == 0) {
      r.dirty[j] = 0, r.evaluated[j] = 1, r.ever[j] = 1, r.parity[j] ^= 1, r.ohead[j] = r.ihead[j];
      atomicAdd(&r.spread[(blockIdx.x % SPREAD) * 8], 1ULL);
    }
#ifdef PGX_BIG_STATS
    uint32_t st_passes = 0, st_rows = 0, st_cut = 0, st_cont = 0, st_multi = 0, st_pairs = 0;   // (Counters, pgx_replay.h)
    unsigned long long st_t0 = 0, st_t1 = 0, st_t2 = 0;
    if (threadIdx.x == 0) st_t0 = wall_clock64();
#endif
    // ---- LOOK: the triangle of pairs (row i, partner p > i), folded into n / 2 lines of n (row f in front, row n - 2 - f behind it) ----
    {
      const uint32_t total = (n >> 1) * n;
      for (uint32_t base = 0; base < total; base += LOOK_NB * blockDim.x) {
        uint32_t row[LOOK_NB], par[LOOK_NB], at[LOOK_NB], own[LOOK_NB];
        unsigned long long pair[LOOK_NB];
        bool inb[LOOK_NB], live[LOOK_NB];
#pragma unroll
        for (int k = 0; k < LOOK_NB; ++k) {
          const uint32_t idx = base + (uint32_t)k * blockDim.x + threadIdx.x;
          const uint32_t f = idx / n, c = idx - f * n;
          inb[k] = idx < total;
          if (c < n - 1 - f) row[k] = f, par[k] = f + 1 + c;
          else row[k] = n - 2 - f, par[k] = c, inb[k] = inb[k] && row[k] != f;   // (that row's partners sit at their own columns; the middle row of an odd n - 1 only once)
          uint32_t rid0 = 0, rid1 = 0;
          if (inb[k]) rid0 = s_rid[row[k]], rid1 = s_rid[par[k]];
          live[k] = inb[k] && rid0 != rid1;
          pair[k] = rid0 < rid1 ? ((unsigned long long)rid0 << 32 | rid1) : ((unsigned long long)rid1 << 32 | rid0);
          at[k] = (uint32_t)mix64(pair[k]) & r.pmask, own[k] = 0;
        }
        uint8_t fact[LOOK_NB];
        bool absent[LOOK_NB];
#pragma unroll
        for (int k = 0; k < LOOK_NB; ++k) fact[k] = live[k] ? FACT_VALID : 0, absent[k] = live[k];
#ifdef PGX_BIG_STATS
#pragma unroll
        for (int k = 0; k < LOOK_NB; ++k) st_pairs += live[k] ? 1u : 0u;
#endif
        // pair_find of the LOOK_NB pairs: an iteration loads the slot of every one of them (a finished one its last slot again) and then tests
        for (int probes = 0; probes < 1024; ++probes) {
          uint4 h[LOOK_NB];
#pragma unroll
          for (int k = 0; k < LOOK_NB; ++k) h[k] = *reinterpret_cast<const uint4 *>(&r.ph[at[k]]);
          bool more = false;
#pragma unroll
          for (int k = 0; k < LOOK_NB; ++k) {
            if (!live[k]) continue;
            const unsigned long long key = (unsigned long long)h[k].y << 32 | h[k].x;
            if (key == pair[k] + 1) own[k] = h[k].z, live[k] = false;
            else if (key == 0) live[k] = false;
            else at[k] = (at[k] + 1) & r.pmask, more = true;
          }
          if (!more) break;
        }
        uint32_t q_off[LOOK_NB], rlen0[LOOK_NB], rlen1[LOOK_NB], mb[LOOK_NB], req[LOOK_NB];
        unsigned long long ma[LOOK_NB];
        bool unfiled[LOOK_NB];
#pragma unroll
        for (int k = 0; k < LOOK_NB; ++k) {
          const bool present = own[k] != 0 && own_bucket(own[k]) < j;
          if (present) fact[k] |= FACT_PRESENT | (uint8_t)(own_type(own[k]) << FACT_TYPE_SHIFT);
          absent[k] = absent[k] && !present;
          q_off[k] = rlen0[k] = rlen1[k] = mb[k] = 0, ma[k] = 0, req[k] = NONE, unfiled[k] = true, at[k] = 0;
          if (absent[k]) {
            const uint32_t dir0 = s_dir[row[k]], dir1 = s_dir[par[k]];
            rlen0[k] = s_rl[row[k]], rlen1[k] = s_rl[par[k]];
            q_off[k] = s_pos[row[k]] - s_pos[par[k]];
            if (q_off[k] >= (1u << 30)) atomicOr(&r.c->overflow, OV_QOFF);
            ma[k] = (unsigned long long)s_rid[row[k]] << 32 | s_rid[par[k]], mb[k] = q_off[k] << 2 | dir0 << 1 | dir1;
            at[k] = (uint32_t)mix64(ma[k] ^ mix64(mb[k])) & r.mmask;
          }
          live[k] = absent[k] && r.memo_used != 0;
        }
        if (r.memo_used) {   // memo_find of the absent ones, in the same form
          for (int probes = 0; probes < 1024; ++probes) {
            uint4 h[LOOK_NB];
#pragma unroll
            for (int k = 0; k < LOOK_NB; ++k) h[k] = *reinterpret_cast<const uint4 *>(&r.mt[at[k]]);
            bool more = false;
#pragma unroll
            for (int k = 0; k < LOOK_NB; ++k) {
              if (!live[k]) continue;
              const unsigned long long cur = (unsigned long long)h[k].y << 32 | h[k].x;
              if (cur == 0) live[k] = false;
              else if (cur == ma[k] && h[k].z == mb[k] + 1) req[k] = h[k].w, unfiled[k] = false, live[k] = false;
              else at[k] = (at[k] + 1) & r.mmask, more = true;
            }
            if (!more) break;
          }
        }
        pgx_match res[LOOK_NB];   // the settled results, all loaded before the first is classified
#pragma unroll
        for (int k = 0; k < LOOK_NB; ++k)
          if (absent[k] && req[k] < r.settled) res[k] = r.rq_res[req[k]];
#pragma unroll
        for (int k = 0; k < LOOK_NB; ++k) {
          if (absent[k]) {
            bool accepted, guessed = false;
            uint32_t type;
            if (req[k] < r.settled) {
              accepted = classify(res[k], rlen0[k], rlen1[k], q_off[k], &type);
            } else {
              accepted = true, guessed = true, type = T_OVERLAP;
              if (r.predict && predict_contained(rlen0[k], rlen1[k], q_off[k], r.predict, r.predict2)) type = rlen0[k] >= rlen1[k] ? T_CONTAINS : T_CONTAINED;
            }
            fact[k] |= (uint8_t)((accepted ? FACT_ACCEPTED : 0) | (guessed ? FACT_GUESSED : 0) | (unfiled[k] ? FACT_UNFILED : 0) | type << FACT_TYPE_SHIFT);
          }
          if (inb[k]) s_fact[row[k] * 128 + par[k]] = fact[k];
        }
      }
    }
    __syncthreads();   // (the facts are there)
#ifdef PGX_BIG_STATS
    if (threadIdx.x == 0) st_t1 = wall_clock64();
#endif
    // ---- WALK: wavefront 0, no global access and no barrier from here to its end ----
    // The rows in order (n - 2 downwards, skipping those an earlier row flagged contained), each over its partners in ascending order, 64 per pass:
    // lane l looks at partner first + l.  The state is uniform -- ballots and what follows from them -- and lives in scalar registers.  A row
    // takes another pass when this one neither reached best-n nor ended the row, or when it was cut at a duplicate; `got` carries over.
    if (__builtin_amdgcn_readfirstlane(w) == 0) {
      __builtin_amdgcn_s_setprio(3);   // (the launch waits for this one wavefront: it goes first where the narrow kernel's wavefronts share the CU)
      uint64_t clo = 0, chi = 0;   // "contained" flags of the bucket's entries
      uint32_t num = 0, lookups = 0, skips = 0;
      bool any_guess = false, any_unfiled = false, bail = false;
      uint32_t set_n = 0;          // pairs in the LDS set so far
      int row = (int)n - 1;        // rows >= row are finished (the first row is n - 2)
      while (r.bestn != 0 && !bail) {
        {   // the next row below that is not contained
          const M128 below{row >= 64 ? ~0ULL : (1ULL << row) - 1ULL, row > 64 ? (1ULL << (row - 64)) - 1ULL : 0ULL};   // (selects, not branches; row <= 127)
          const M128 open = andn128(below, M128{clo, chi});
          if (!any128(open)) break;
          row = open.hi ? 127 - __builtin_clzll(open.hi) : 63 - __builtin_clzll(open.lo);
        }
        uint32_t first = (uint32_t)row + 1, got = 0;
        M128 vis{0, 0}, ins{0, 0};   // the row's partners (bit = entry index) visited / inserted, over all its passes
        const uint32_t row_twice = dup ? (uint32_t)__builtin_amdgcn_readfirstlane((int)s_same[row]) & 0x100u : 0u;   // the row's read stands in the bucket again
#ifdef PGX_BIG_STATS
        uint32_t row_passes = 0;
#endif
        for (;;) {
          const uint32_t pi = first + (uint32_t)lane;
          // partners of this pass that an earlier row flagged contained: not looked at.  (bits first .. first + 63 of the flags; 1 <= first <= 127)
          const uint64_t gone = first < 64 ? clo >> first | (chi << 1) << (63 - first) : chi >> (first - 64);
          uint32_t fact = 0, same = 0;
          if (pi < n) {
            fact = s_fact[row * 128 + (int)pi];
            if (dup) same = s_same[pi];
          }
          // the pair can be met twice in this evaluation only if one of its reads stands in the bucket twice: only such pairs are looked for in the
          // set, and noted there when inserted
          const bool twice = pi < n && ((row_twice | same) & 0x100u) != 0;
          unsigned long long pair = 0;
          if (twice) {
            const uint32_t rid0 = s_rid[row], rid1 = s_rid[pi];
            pair = rid0 < rid1 ? ((unsigned long long)rid0 << 32 | rid1) : ((unsigned long long)rid1 << 32 | rid0);
          }
          if (set_n) {   // a pair LOOK found absent: inserted earlier in THIS evaluation?  Then it is present, with the type noted in the set
            if (twice && (fact & (FACT_VALID | FACT_PRESENT)) == FACT_VALID) {
              for (uint32_t i = (uint32_t)mix64(pair) & (SET_CAP - 1);; i = (i + 1) & (SET_CAP - 1)) {
                const unsigned long long kk = s_setk[i];
                if (kk == 0) break;
                if (kk == pair + 1) {
                  fact = FACT_VALID | FACT_PRESENT | (uint32_t)s_sett[i] << FACT_TYPE_SHIFT;
                  break;
                }
              }
            }
          }
          // a ballot per bit of the fact and per type (one compare each), combined as scalars
          const uint32_t ty = fact >> FACT_TYPE_SHIFT;
          const uint64_t mv = __ballot((fact & FACT_VALID) != 0) & ~gone;        // looked at
          const uint64_t mp = __ballot((fact & FACT_PRESENT) != 0) & mv;         // seen: skipped
          const uint64_t ma = __ballot((fact & FACT_ACCEPTED) != 0) & mv & ~mp;  // would be inserted
          const uint64_t mto = __ballot(ty == T_OVERLAP), mtc = __ballot(ty == T_CONTAINED), mtp = __ballot(ty == T_CONTAINS);
          const uint64_t mgu = __ballot((fact & FACT_GUESSED) != 0), muf = __ballot((fact & FACT_UNFILED) != 0);
          const uint64_t inc = (mp | ma) & mto;   // counts towards best-n
          const uint64_t ac = ma & mtc;           // the row's read is contained: the row ends there
          const uint64_t ap = ma & mtp;           // the partner is contained
          // two partners of the pass with the same read (dup buckets): a lane that found its pair absent is flagged when a LOWER lane of the pass
          // would insert the same pair -- that is, holds the same read: s_same leads from an entry to the earlier ones of its read.  That holds
          // also for a lane whose own alignment is rejected: sequentially it would have found the pair seen.  The row is cut in front of the
          // first flagged lane, which the next pass looks at again and then finds in the set.
          uint64_t df = 0;
          const uint64_t absent = mv & ~mp;
          if (dup && ma && (absent & (absent - 1))) {
            bool dflag = false;
            if ((absent >> lane) & 1) {
              for (uint32_t p = same & 0xFFu; p > first; p = s_same[p - 1] & 0xFFu)   // (entry p - 1 >= first: lane p - 1 - first of this pass)
                if ((ma >> (p - 1 - first)) & 1) {
                  dflag = true;
                  break;
                }
            }
            df = __ballot(dflag);
          }
          const int cut = df ? (int)__builtin_ctzll(df) : 64;   // first lane that may not be processed (>= 1: lane 0 has no lower lane)
          const uint32_t need = r.bestn - got;                  // >= 1
          int stop = 64;
          if ((uint32_t)__popcll(inc) >= need) stop = nth64(inc, need);
          if (ac) stop = min(stop, (int)__builtin_ctzll(ac));
          const bool ends = stop < cut;   // the row ends within this pass, in front of the cut
          const int last = ends ? stop : cut - 1;
          const uint64_t proc = last >= 63 ? ~0ULL : (2ULL << last) - 1ULL;   // the lanes the walk really processes
          const uint64_t pv = mv & proc, pins = ma & proc, apk = ap & proc;
          num += (uint32_t)__popcll(pins), skips += (uint32_t)__popcll(mp & proc), lookups += (uint32_t)__popcll(pv & ~mp);
          got += (uint32_t)__popcll(inc & proc);
          any_guess |= (mgu & pins) != 0, any_unfiled |= (muf & pins) != 0;
          auto up = [&](uint64_t m) { return first < 64 ? M128{m << first, (m >> 1) >> (63 - first)} : M128{0, m << (first - 64)}; };   // lanes -> entry indices
          vis = or128(vis, up(pv)), ins = or128(ins, up(pins));
          {   // partners found contained
            const M128 c = up(apk);
            clo |= c.lo, chi |= c.hi;
          }
          if (ac & proc) {   // the row's own read
            if (row < 64) clo |= 1ULL << row;
            else chi |= 1ULL << (row - 64);
          }
#ifdef PGX_BIG_STATS
          ++st_passes, ++row_passes, st_cut += (!ends && cut < 64) ? 1u : 0u, st_cont += (ac & proc) ? 1u : 0u;
#endif
          const uint64_t pset = __ballot(twice) & pins;
          if (pset) {   // this evaluation's insertions that can be met again, for the probes of the passes to come
            bool full = false;
            set_n += (uint32_t)__popcll(pset);
            if ((pset >> lane) & 1) {
              uint32_t tries = 0;
              for (uint32_t i = (uint32_t)mix64(pair) & (SET_CAP - 1);; i = (i + 1) & (SET_CAP - 1)) {
                const unsigned long long kk = atomicCAS(&s_setk[i], 0ULL, (unsigned long long)pair + 1);
                if (kk == 0 || kk == pair + 1) {
                  s_sett[i] = (uint8_t)ty;
                  break;
                }
                if (++tries >= SET_CAP) {   // the set is full (not with <= 128 entries and bestn <= ~8; kept as a guard): leave the bucket to k_eval_rows
                  full = true;
                  break;
                }
              }
            }
            BIG_WAVE_SYNC();
            bail = __ballot(full) != 0;
          }
          first += (uint32_t)(cut < 64 ? cut : 64);
          if (ends || bail || first >= n) break;
        }
        if (lane == 0 && any128(vis)) s_vis[row] = vis, s_ins[row] = ins;   // (the row is complete: its masks, once)
#ifdef PGX_BIG_STATS
        ++st_rows, st_multi += row_passes > 1 ? 1u : 0u;
#endif
      }
      __builtin_amdgcn_s_setprio(0);
      if (lane == 0) s_walk[0] = num, s_walk[1] = lookups, s_walk[2] = skips, s_walk[3] = (any_guess ? 1u : 0u) | (any_unfiled ? 2u : 0u), s_bail = bail ? 1u : 0u;
    }
    __syncthreads();   // (the walk is over: the rows' masks and s_walk are there)
    const uint32_t num = s_walk[0], lookups = s_walk[1], skips = s_walk[2];
    const bool any_guess = (s_walk[3] & 1) != 0, any_unfiled = (s_walk[3] & 2) != 0;
    uint32_t head = NIL;
    // ---- COMMIT (not on the guard path: nothing has been written for the bucket then) ----
#ifdef PGX_BIG_STATS
    if (threadIdx.x == 0) st_t2 = wall_clock64();
#endif
    bool p_reg = false;          // this lane has a registration whose list position (p_idx) has not been looked at yet
    uint32_t p_idx = 0, p_slot = 0;
    auto resolve_pending = [&]() {   // as in k_eval_rows; an exhausted arena raises s_abort instead of returning
      if (p_reg && p_idx < NIN) r.pc[p_slot >> r.cshift].in[p_idx] = j + 1, p_reg = false;
      const uint64_t rm = __ballot(p_reg);
      if (rm) {
        const uint32_t total = (uint32_t)__popcll(rm);
        if (rcur + total > rend) {
          uint32_t base = 0;
          if (lane == 0) base = atomicAdd(&r.c->rnode_top, NCH);
          base = (uint32_t)__shfl((int)base, 0, 64);
          if ((uint64_t)base + NCH > r.rn_cap) {
            atomicOr(&r.c->overflow, OV_NODES);
            s_abort = 1;
            p_reg = false;
            return;
          }
          rcur = base, rend = base + NCH;
        }
        if (p_reg) {
          const uint32_t node = rcur + lane_rank(rm);
          const uint32_t old = atomicExch(&r.pc[p_slot >> r.cshift].rhead, node + 1);
          r.rn[node] = RNode{old, j};
        }
        rcur += total;
        p_reg = false;
      }
    };
    if (!s_bail) {
      // the rows' first insertion ordinals: a prefix count over the inserted masks in walk order (row n - 2 first)
      if (threadIdx.x < 128) {
        const int row = (int)n - 2 - (int)threadIdx.x;
        const uint32_t c = row >= 0 ? (uint32_t)popc128(s_ins[row]) : 0u;
        uint32_t incl = c;
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
          if (lane >= o) incl += up;
        }
        if (lane == 63) s_wsum[w] = incl;
        if (row >= 0) s_rbase[row] = incl - c;   // (the second wavefront's rows: + s_wsum[0], added where it is read)
      }
      if (threadIdx.x == 0 && num) {   // the item chunks of the evaluation: one allocation for the workgroup, by thread 0
        const uint32_t want = 16u * ((num + 15) >> 4);
        if (icur + want > iend) {
          const uint32_t take = want > ICH ? want : ICH;
          const uint32_t base = atomicAdd(&r.c->item_top, take);
          if ((uint64_t)base + take > r.item_cap) atomicOr(&r.c->overflow, OV_ITEMS), s_abort = 1;
          icur = base, iend = base + take;
        }
        s_fresh = icur, icur += want;
      }
      __syncthreads();   // (s_rbase, s_wsum, s_fresh)
      if (!s_abort) {
        const uint32_t fresh = s_fresh;   // the chunks are consecutive: the item of ordinal o is fresh + o
        const int half = w & 1;
        for (int row = (int)n - 2 - (w >> 1); row >= 0; row -= BIG_NR) {   // a wavefront per (row, half of its partners)
          const uint64_t vm = half ? s_vis[row].hi : s_vis[row].lo, im = half ? s_ins[row].hi : s_ins[row].lo;
          if (!vm) continue;
          const uint32_t pi = (uint32_t)(half * 64 + lane);
          bool reg = ((vm >> lane) & 1) != 0;   // the partners the walk really examined register as readers of their pairs (as in k_eval_rows)
          const bool my_ins = ((im >> lane) & 1) != 0;
          uint32_t slot = NONE, rid0 = 0, rid1 = 0;
          if (reg) {
            rid0 = s_rid[row], rid1 = s_rid[pi];
            slot = pair_slot(r, rid0 < rid1 ? ((uint64_t)rid0 << 32 | rid1) : ((uint64_t)rid1 << 32 | rid0));
          }
          uint32_t mslot = NONE;
          const uint32_t fact = my_ins ? s_fact[row * 128 + (int)pi] : 0u;
          if (my_ins && !(fact & FACT_UNFILED)) {
            uint32_t req;
            mslot = memo_find(r, (unsigned long long)rid0 << 32 | rid1, (s_pos[row] - s_pos[pi]) << 2 | (uint32_t)s_dir[row] << 1 | s_dir[pi], &req);
          }
          resolve_pending();   // (the previous row's registrations: their atomics have returned behind the loads above)
          if (reg && !first_eval) {
            const uint32_t *pw = reinterpret_cast<const uint32_t *>(&r.pc[slot >> r.cshift]);
            const uint4 h1 = *reinterpret_cast<const uint4 *>(pw);  // cnt, rhead, in[0], in[1]
            const uint32_t c = min(h1.x, NIN);
            if ((c > 0 && h1.z == j + 1) || (c > 1 && h1.w == j + 1)) reg = false;
            for (uint32_t qq = 2; qq < c && reg; qq += 8) {
              const uint4 xa = *reinterpret_cast<const uint4 *>(pw + 2 + qq), xb = *reinterpret_cast<const uint4 *>(pw + 6 + qq);
              const uint32_t x[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
              for (uint32_t k = 0; k < 8; ++k)
                if (qq + k < c && x[k] == j + 1) reg = false;
            }
          }
          if (reg) p_idx = atomicAdd(&r.pc[slot >> r.cshift].cnt, 1u), p_slot = slot, p_reg = true;
          if (my_ins) {
            const uint32_t ord = s_rbase[row] + ((int)n - 2 - row >= 64 ? s_wsum[0] : 0u) + (half ? (uint32_t)__popcll(s_ins[row].lo) : 0u) +
                                 (uint32_t)__popcll(im & ((1ULL << lane) - 1ULL));   // insertion ordinal within the bucket
            const uint32_t idx = fresh + ord;
            uint32_t info = (uint32_t)row | pi << 8 | (fact >> FACT_TYPE_SHIFT) << 16;
            if (fact & FACT_GUESSED) info |= I_GUESS;
            if (mslot == NONE) info |= I_UNFILED;
            r.items[idx] = Item{slot, info, mslot, ord == 0 ? NIL : idx};   // next: the item before this one, + 1 (also across a chunk's edge)
          }
        }
        if (num) head = fresh + num;   // the last item, + 1
      }
    }
    resolve_pending();
#ifdef PGX_BIG_STATS
    {
      for (int o = 32; o; o >>= 1) st_pairs += (uint32_t)__shfl_xor((int)st_pairs, o, 64);
      if (lane == 0) atomicAdd(&r.c->big_pairs, (unsigned long long)st_pairs);
    }
    if (threadIdx.x == 0) {   // [3] row passes, [4] rows completed, [5] passes cut at a duplicate, [6] rows ended by a containment, [7] rows of more than one pass
      unsigned long long *line = r.spread + (blockIdx.x % SPREAD) * 8;
      atomicAdd(line + 3, (unsigned long long)st_passes), atomicAdd(line + 4, (unsigned long long)st_rows), atomicAdd(line + 5, (unsigned long long)st_cut);
      atomicAdd(line + 6, (unsigned long long)st_cont), atomicAdd(line + 7, (unsigned long long)st_multi);
      atomicMax(&r.c->big_max_passes, st_passes);
      if (st_passes >= 64) atomicAdd(&r.c->big_long, 1u), atomicAdd(&r.c->big_long_n, n);
      atomicAdd(&r.c->big_evals, 1u);
      const unsigned long long t3 = wall_clock64(), tl = st_t1 - st_t0, tw = st_t2 - st_t1, tc = t3 - st_t2;   // the phases, and the launch's longest evaluation
      atomicAdd(&r.c->big_cyc[0], tl), atomicAdd(&r.c->big_cyc[1], tw), atomicAdd(&r.c->big_cyc[2], tc);
      atomicMax(&r.c->big_lmax, (t3 - st_t0) << 40 | (tw & 0xFFFFF) << 20 | (tl & 0xFFFFF));
    }
#endif
    if (threadIdx.x == 0) {
      if (s_bail) {   // (guard path: evaluated again by k_eval_rows, one partner at a time; COMMIT was skipped, so nothing of this evaluation is left)
        r.dirty[j] = 1, r.evaluated[j] = 0, r.parity[j] ^= 1;
        r.bflags[j] = (uint8_t)((r.bflags[j] & ~F_BIG));
      } else {
        r.ihead[j] = head, r.inum[j] = num, r.lookups[j] = lookups, r.skips[j] = skips;
        r.bflags[j] = (uint8_t)(F_BIG | (dup ? F_DUP : 0) | (any_guess ? F_GUESS : 0) | (any_unfiled ? F_UNFILED : 0));
      }
    }
  }
  if (s_abort) break;
  }
  if (lane == 0) r.wcur[wave_id] = make_uint4(rcur, rend, icur, iend);
#ifdef PGX_BIG_STATS
  if (threadIdx.x == 0) {   // the last workgroup of the launch adds the launch's longest evaluation to the sums
    __threadfence();
    if (atomicAdd(&r.c->big_ticket, 1u) == gridDim.x - 1) {
      const unsigned long long m = atomicExch(&r.c->big_lmax, 0ULL);
      if (m) {
        const unsigned long long tl = m & 0xFFFFF, tw = (m >> 20) & 0xFFFFF;
        r.c->big_cyc_long[0] += tl, r.c->big_cyc_long[1] += tw, r.c->big_cyc_long[2] += (m >> 40) - tl - tw, r.c->big_launches += 1;
      }
      r.c->big_ticket = 0;
    }
  }
#endif
}
#undef BIG_WAVE_SYNC

}  // namespace rp
}  // namespace pgx
