// k_rq_draw: GoGameTrain::act's draws (elfrq_draw, record_host.cpp, is the specification) on the GPU, and k_rq_scatter, which keeps
// the queue mirror they read up to date.  DESIGN.md section 3 has the layout, the speculation scheme and the cost model.
//
// One workgroup of one wavefront per game thread.  The thread's std::mt19937 lives in LDS as TWO consecutive raw blocks of 624
// words (block `cur` holds the stream position, the other one is its successor), so that an output is addressable by its
// position up to 1248 - pos ahead and a state's draws may straddle a block boundary; outputs are tempered when read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rq {

constexpr int MT_N = 624, MT_M = 397;
constexpr int NUM_STATE = 64;            // kNumState: states per act, one lane each
constexpr int MAX_TRIES = 1 << 20;       // elfrq_draw's bound on the tries of one state
constexpr int MAX_QUEUES = 4096;         // head and size of every queue sit in LDS: 32 KB at the most
constexpr int CHUNK = 1024;              // records per mirror update launch

// The mirror: queue i's deque element j is ring[i * qmax + (head[i] + j) % qmax] = (slot, num_moves)
struct Mirror {
  int2* ring;
  int32_t* head;
  int32_t* size;
  int nq, qmax, qmin;
};

// One update: chunk = { n, head[nq], size[nq], pad to 4 ints, n x (queue, ring position, slot, num_moves) } in device memory
__host__ __device__ inline int chunk_entries_at(int nq) { return (1 + 2 * nq + 3) & ~3; }

__global__ void k_rq_scatter(Mirror m, const int32_t* __restrict__ chunk) {
  const int n = chunk[0];
  const int4* e = reinterpret_cast<const int4*>(chunk + chunk_entries_at(m.nq));
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n || i < m.nq; i += gridDim.x * blockDim.x) {
    if (i < m.nq) { m.head[i] = chunk[1 + i]; m.size[i] = chunk[1 + m.nq + i]; }
    if (i < n) {
      const int4 v = e[i];
      if (v.x >= 0 && v.x < m.nq && v.y >= 0 && v.y < m.qmax) m.ring[(size_t)v.x * m.qmax + v.y] = make_int2(v.z, v.w);
    }
  }
}

__device__ inline uint32_t mt_mix(uint32_t a, uint32_t b) {
  const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
  return (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// mersenne_twister_engine::_M_gen_rand from block S into block D, by the whole wave: words 0..226 need old words only, 227..453
// the new 0..226, 454..623 the new 227..396 (and word 623 the new word 0) -- three phases of four, four and three 64-lane steps.
__device__ inline void mt_twist(const uint32_t* S, uint32_t* D, int lane) {
  for (int i = lane; i < MT_N - MT_M; i += 64) D[i] = S[i + MT_M] ^ mt_mix(S[i], S[i + 1]);
  __syncthreads();
  for (int i = MT_N - MT_M + lane; i < 2 * (MT_N - MT_M); i += 64) D[i] = D[i - (MT_N - MT_M)] ^ mt_mix(S[i], S[i + 1]);
  __syncthreads();
  for (int i = 2 * (MT_N - MT_M) + lane; i < MT_N; i += 64) D[i] = D[i - (MT_N - MT_M)] ^ mt_mix(S[i], i == MT_N - 1 ? D[0] : S[i + 1]);
  __syncthreads();
}

struct Gen {
  uint32_t* raw;   // LDS, [2][624]
  int cur;         // the block the stream position is in
  int pos;         // the position in it: < 624 after settle()
  // the tempered output `p` words past the start of block cur, p < 1248
  __device__ uint32_t at(int p) const {
    int i = p + cur * MT_N;
    if (i >= 2 * MT_N) i -= 2 * MT_N;
    uint32_t z = raw[i];
    z ^= z >> 11;
    z ^= (z << 7) & 0x9d2c5680u;
    z ^= (z << 15) & 0xefc60000u;
    z ^= z >> 18;
    return z;
  }
  // wave-uniform: moves on to the block the position has reached and makes that block's successor
  __device__ void settle(int lane) {
    while (pos >= MT_N) {
      cur ^= 1;
      pos -= MT_N;
      mt_twist(raw + cur * MT_N, raw + (cur ^ 1) * MT_N, lane);
    }
  }
};

// One try of one state, from stream position p (elfrq_draw's loop body): kind 0 = a record, 5 outputs used (the state's d4 is the
// sixth); 1 = the queue is below queue_min_size, 3 used; 2 = the record is shorter than num_future_actions, 4 used.
struct Try { int kind; int32_t slot, move_to; };

__device__ inline Try draw_try(const Gen& g, int p, const Mirror& m, const int32_t* s_head, const int32_t* s_size, int nfa, float even_ratio) {
  Try t{1, 0, 0};
  int idx = 2 * (int)(g.at(p) % (uint32_t)(m.nq / 2));
  // std::generate_canonical<double, 53> over a 32-bit engine (bits/random.tcc): two outputs, the low word first, summed in
  // double with one rounding, over 2^64; nextafter(1, 0) if that rounds to 1.  uniform_real(0, 1) returns it as it is.
  const double lo = (double)g.at(p + 1), hi = (double)g.at(p + 2);
  double u = (lo + hi * 4294967296.0) / 18446744073709551616.0;
  if (u >= 1.0) u = 0x1.fffffffffffffp-1;
  if (u > (double)even_ratio) idx++;
  const int sz = s_size[idx];
  if (sz < m.qmin) return t;
  int at = s_head[idx] + (int)(g.at(p + 3) % (uint32_t)sz);
  if (at >= m.qmax) at -= m.qmax;
  const int2 r = m.ring[(size_t)idx * m.qmax + at];
  t.kind = 2;
  if (r.y <= nfa - 1) return t;
  t.kind = 0;
  t.slot = r.x;
  t.move_to = (int32_t)(g.at(p + 4) % (uint32_t)(r.y - nfa + 1));
  return t;
}

// grid = game threads, block = 64.  mt: [T][624] raw state words, mt_pos: [T] position (0..624, as std::mt19937 keeps it).
// Act a of the call belongs to thread (first + a) % T and writes outputs a * 64 .. a * 64 + 63.
__global__ void __launch_bounds__(64) k_rq_draw(Mirror m, uint32_t* __restrict__ mt, uint32_t* __restrict__ mt_pos, int T, int first,
                                                int num_acts, int nfa, float even_ratio, int32_t* __restrict__ out_slot,
                                                int32_t* __restrict__ out_move_to, int32_t* __restrict__ out_d4, uint32_t* __restrict__ stuck) {
  __shared__ uint32_t s_raw[2 * MT_N];
  __shared__ int32_t s_out[3][NUM_STATE];
  extern __shared__ int32_t s_queues[];   // head[nq], size[nq]
  const int tt = blockIdx.x, lane = threadIdx.x;
  const int a0 = ((tt - first) % T + T) % T;
  if (a0 >= num_acts) return;             // no act in this call: the generator is not touched
  int32_t* s_head = s_queues;
  int32_t* s_size = s_queues + m.nq;
  for (int i = lane; i < m.nq; i += 64) { s_head[i] = m.head[i]; s_size[i] = m.size[i]; }
  for (int i = lane; i < MT_N; i += 64) s_raw[i] = mt[(size_t)tt * MT_N + i];
  Gen g{s_raw, 0, (int)mt_pos[tt]};
  __syncthreads();
  mt_twist(s_raw, s_raw + MT_N, lane);
  g.settle(lane);                         // a position of 624 (a freshly seeded generator) moves on to the successor

  for (int a = a0; a < num_acts; a += T) {
    int done = 0;                         // states of this act that are final
    while (done < NUM_STATE) {
      // every open state speculates that no state before it draws again: state done + lane reads outputs pos + 6 * lane .. + 5
      const bool open = done + lane < NUM_STATE;
      const int p = g.pos + 6 * lane;
      const Try t = draw_try(g, p, m, s_head, s_size, nfa, even_ratio);
      const uint64_t again = __ballot(open && t.kind != 0);
      const int clean = min(again ? __ffsll((unsigned long long)again) - 1 : 64, NUM_STATE - done);   // the lanes below the first retry
      if (lane < clean) {
        s_out[0][done + lane] = t.slot;
        s_out[1][done + lane] = t.move_to;
        s_out[2][done + lane] = (int32_t)(g.at(p + 5) % 8u);
      }
      done += clean;
      g.pos += 6 * clean;
      g.settle(lane);
      if (!again) continue;
      // State `done` draws again: its tries are resolved with their exact consumption.  Up to 64 of them at a time, speculating
      // that each one before ends on a short record (4 outputs): lane l reads pos + 4 * l .. + 4.
      int tries = 0;
      bool found = false;
      while (!found && tries < MAX_TRIES) {
        const int width = min(64, MAX_TRIES - tries);
        const Try r = draw_try(g, g.pos + 4 * lane, m, s_head, s_size, nfa, even_ratio);
        const uint64_t other = __ballot(lane < width && r.kind != 2);
        if (!other) {
          tries += width;
          g.pos += 4 * width;
        } else {
          const int f = __ffsll((unsigned long long)other) - 1;
          found = __shfl(r.kind, f) == 0;
          tries += f + 1;
          g.pos += 4 * f + (found ? 5 : 3);
          if (found && lane == f) { s_out[0][done] = r.slot; s_out[1][done] = r.move_to; }
        }
        g.settle(lane);
      }
      if (lane == 0) {
        if (!found) { s_out[0][done] = 0; s_out[1][done] = 0; *stuck = 1u; }
        s_out[2][done] = (int32_t)(g.at(g.pos) % 8u);
      }
      done += 1;
      g.pos += 1;
      g.settle(lane);
    }
    __syncthreads();
    const size_t o = (size_t)a * NUM_STATE + lane;
    out_slot[o] = s_out[0][lane];
    out_move_to[o] = s_out[1][lane];
    out_d4[o] = s_out[2][lane];
    __syncthreads();
  }
  for (int i = lane; i < MT_N; i += 64) mt[(size_t)tt * MT_N + i] = s_raw[g.cur * MT_N + i];
  if (lane == 0) mt_pos[tt] = (uint32_t)g.pos;
}

}  // namespace rq
