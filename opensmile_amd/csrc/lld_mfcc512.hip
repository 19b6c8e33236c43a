// Fast fused MFCC kernel for Nfft = 512 (16 kHz, 20..32 ms frames) on gfx950.
//
// Mapping (wave64-native): ONE WAVE processes FOUR frames at a time, 16 lanes
// per frame; a wave walks a tile of consecutive frames of one utterance in
// "passes" of 4 frames. Waves are autonomous -- no __syncthreads in the frame
// loop, all exchange is wave-local (LDS or DPP). Sized for 4 waves per SIMD
// (<= 128 VGPRs, ~8 KB of LDS per wave): one wave can issue a VALU op only
// every ~5 cycles (tools/ubench/valu_rate.hip), so the SIMD needs several
// waves to approach its ~2.5-cycle issue rate.
//
// Per pass (lane j = lane&15 of group g = lane>>4, frame t = tp + g):
//   load    lane (g, j) loads from global memory exactly the sample pairs it
//           transforms -- pair n = j + 16 m of frame t, m < MP -- one pass ahead
//           (the 2.5x overlap of the frames is served by L1/L2; no LDS stage).
//           The loads are TYPED buffer loads (round 9): the buffer unit hands the int16 samples over
//           as floats, so the conversion costs no vector instruction (the PLP chain and the
//           delta-fused MP = 16 instances keep integer loads and convert on the vector ALU:
//           typed_loads() below).
//           Conversion (R0, scale folded into the window table), pre-emphasis
//           (R2, one fused multiply-add; the previous sample comes from
//           the neighbour lane by DPP) and window (R3) happen in registers:
//           z[m] = y[2n] + i*y[2n+1]; the real 512-FFT is a complex 256-FFT of z
//           plus an untangle pass
//   FFT     256 = 16 x 16: radix-16 DFT over m in registers (two radix-4
//           layers, constants only), twiddle by w256^(j*k1) (LDS table), ONE
//           16x16 transpose through LDS (a plane of re and a plane of im: address-free
//           b32 stores, b128 loads, conflict-free by a table of row bases: kTSWaveFloats), radix-16 DFT over j
//           Order of the transposition traffic (round 8): the first DFT's last layer finishes its outputs in groups of four --
//           k1 = 0, 4, 8, 12, then 1, 5, 9, 13, .. -- and each is twiddled and stored at once, so the sixteen stores are spread
//           over that layer and the twiddles instead of standing in one block in front of the sixteen loads (which are issued
//           in index order jj = 0 .. 15). LDS operations
//           of a wave return in order: what a wave waits for is decided by the ORDER of its requests. No instruction is added,
//           and an instruction's lane -> bank pattern does not depend on its position (tools/lds_bank_sim.py)
//   spect.  columns c and 16-c own mirror-image bins. Lane j transforms column kc(j) = 0 .. 7, 9 .. 15, 8 (it reads that column of
//           the transposition buffer; its twiddles and its places in the power buffer go by kc too), so lanes i and 15-i hold
//           partner columns: the partner's half of Z arrives by ONE DPP step (row_mirror), in place; lane 15 (column 8) and lane 0
//           (column 0) are their own partners, lane 0 one register up (untangle_partner). The PLP chain and the delta-fused MP = 16
//           instances keep kc = j and three DPP steps (one_hop_exchange()). BOTH X[k] and
//           X[256-k] are untangled from one (Z[k], Z[256-k]) pair (R4), power
//           (R5, R6's square) -> LDS power buffer (octets of bins, 12 floats apart)
//   mel     R6 as table-driven work units: a unit = one aligned octet of bins
//           x one band (8 weights, zero outside the band): 2 x ds_read_b128 of
//           power + 2 x b128 of weights + 8 FMA. Whole bands are dealt to the 16
//           lanes, at most two per lane and UC (6 or 8) units per lane, so a band
//           is summed in registers in unit order and its lane takes the log; the
//           unit offsets are loop-invariant registers and the host orders every
//           lane's units so that the 16 lanes of a frame read 16 different bank
//           quads at each step (fast512_build_host)
//   cep     DCT-II rows + lifter (R7): one lane per coefficient, b128 reads
//
// Numerics: R3 keeps the reference's rounding on integer-valued samples (the
// 1/32767 of R0 is folded into the window table, <= 1 ulp per sample); R2 is
// one fused multiply-add per sample since round 6 (one rounding, not two); the FFT uses FMA and its own butterfly order (cannot match Ooura's
// split radix anyway); power skips the reference's sqrt-then-square; mel/DCT
// sums use FMA in a fixed deterministic order. Deviation from the reference is
// measured in tests/test_gpu_mfcc.py; the reference-order path is
// lld_mfcc_generic (SMILEHIP_FORCE_GENERIC=1).
#include <hip/hip_runtime.h>
#include "kernel_timing.hpp"
#include "phase_timing.hpp"
#include "wave_lifetimes.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "lld_device.hpp"
#include "lld_launch.hpp"
#include "lld_params.hpp"
#include "tables.hpp"

namespace smilehip {

namespace {

constexpr int kWavesPerBlock = 8;
constexpr int kTileFrames = 32;       // frames per wave tile (8 passes)
constexpr int kTB2Row = 65;           // float2 per 4-group row of the transpose buffer (520 B)
constexpr int kTB2Floats = 2 * (15 * kTB2Row + 3 * 16 + 16);   // 2078 floats: footprint of the transpose buffer
constexpr int kLmelFloats = 68;       // per frame group: log-mel [32] | PLP acf [16] | PLP cepstra [16] | 4 floats that move the next
                                      // group's vector one bank quad on: a b128 lane group spans two frame groups, whose
                                      // broadcast reads of the DCT met on one quad at 64 (tools/lds_bank_sim.py)
constexpr int kOctetFloats = 12;      // an octet of power bins starts every 12 floats: octet o sits on bank quad 3 o mod 16
constexpr int kPbFloats = 448;        // power buffer of one frame group (33 octets = 396 floats) rounded to a multiple of 64
                                      // dwords: the four groups of a wave see the same banks
constexpr int kWaveFloats = 2080;     // per-wave LDS: max(transpose buffer, 4 x (kLmelFloats + kPbFloats) = 2064), 16-byte multiple

static_assert(kWaveFloats >= kTB2Floats && kWaveFloats >= 4 * (kLmelFloats + kPbFloats) && kWaveFloats % 4 == 0, "per-wave LDS region");

// The SPLIT-COMPLEX transposition buffer (the instances of split_transpose() below): a plane of real and a plane of imaginary parts,
// a row = the 64 floats that the 64 lanes hold for one index k1 of the first DFT16, at `row base + lane`. The writer is lane-linear
// (lane 16 g + j writes column j of group g), so a row is stored by ds_write_addtid_b32 -- address = M0 + immediate + 4 x lane, no
// address register, 2 cycles of the LDS pipe where a ds_write_b64 of the pair takes 6 (its address and two data registers at 2
// cycles each) -- and the reader, lane (g, kc), takes the sixteen columns of row kc of its group with four ds_read_b128 per plane.
// Row bases are a TABLE: a ds_read_b128 lane group holds lanes j = 0 .. 3, 12 .. 15 of one frame group (rows A, through the lane -> column
// map) and j = 4 .. 11 of the next (rows B), whose columns start four bank quads further on. With q(r) = (base(r) / 4) mod 16 the
// loads are conflict-free iff q is one-to-one on A and on B and q(A) u (q(B) + 4) = q(B) u (q(A) + 4) = all sixteen quads, i.e.
// q(A) = q(A) + 8 and q(B) = complement of q(A), minus 4. q(A) = q(B) = {0, 1, 2, 3, 8, 9, 10, 11} is the one family in which a row
// of A and a row of B share a quad; both planes share it too, so FOUR rows (64 quads, a multiple of 16) stand on each quad one behind
// the other -- re A | re B | im A | im B, slot s = 0 .. 7 -- and the padding is what the quad's steps 0 -> 1 -> 2 -> 3 -> 8 -> .. -> 11 take:
// 11 quads in all, 2048 + 44 floats. The imaginary plane lies 128 floats behind the real one in every slot (one address register,
// immediate offsets). tools/lds_bank_sim.py holds the same table and is the judge (tests/test_lds_ledger_split_transpose.py).
// M0 holds 16 bits of LDS byte address, so the per-wave regions of these instances come FIRST in the block's LDS, the shared
// tables behind them.
constexpr int kTSWaveFloats = 2092;   // per-wave LDS of the split-complex instances: 32 rows of 64 floats + 11 bank quads
// ONE table serves both lane -> column maps: rows 0 .. 3 and 12 .. 15 stand first in slots 0 .. 3 and 4 .. 7, rows 4 .. 11 second in
// slots 0 .. 7. Lanes j = 0 .. 3, 12 .. 15 read rows 0 .. 3, 12 .. 15 (kc = j) or 0 .. 3, 13, 14, 15, 8 (the one-hop map), lanes 4 .. 11
// the other eight: in both maps each set meets every slot once, and only the slot decides the quad.
constexpr int tsplit_base(int r, bool imag) {   // float offset of row r (index k1 = column kc) in the wave's region
  const int s = r < 4 ? r : (r < 12 ? r - 4 : r - 8);        // slot
  const bool b = r >= 4 && r < 12;                            // second of the slot's two rows
  return 256 * s + 4 * (s < 4 ? s : s + 4) + (b ? 64 : 0) + (imag ? 128 : 0);
}
static_assert(tsplit_base(11, true) + 64 == kTSWaveFloats, "last row");
static_assert(kTSWaveFloats >= 4 * (kLmelFloats + kPbFloats) && kTSWaveFloats % 4 == 0, "per-wave LDS region, split-complex");
static_assert(4 * (kWavesPerBlock - 1) * kTSWaveFloats < 65536, "a wave's LDS byte address has to fit M0's 16 bits");
static_assert(kPbFloats % 64 == 0 && kPbFloats >= 33 * kOctetFloats, "power buffer");
static_assert(kLmelFloats >= 64 && kLmelFloats % 4 == 0 && (kLmelFloats / 4) % 2 == 1,
              "band vectors: room for the PLP vectors at +32 and +48, 16-byte aligned, neighbouring groups on different bank quads");

constexpr float C1 = 0.92387953251128673848f;   // cos(pi/8)
constexpr float S1 = 0.38268343236508978178f;   // sin(pi/8)
constexpr float R2 = 0.70710678118654752440f;   // sqrt(1/2)

__device__ __forceinline__ void wave_lds_fence() {
  // LDS operations of one wave execute in order; this only stops the compiler
  // from moving LDS accesses across the point.
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// position of power bin k in a frame group's buffer
__host__ __device__ constexpr int pb_pos(int k) { return k + (kOctetFloats - 8) * (k >> 3); }

// forward DFT4 on (a0..a3), in place: X[q] = sum_m a[m] e^{-2 pi i m q / 4}
__device__ __forceinline__ void dft4(float &r0, float &i0, float &r1, float &i1, float &r2, float &i2,
                                     float &r3, float &i3) {
  const float t0r = r0 + r2, t0i = i0 + i2;
  const float t1r = r0 - r2, t1i = i0 - i2;
  const float t2r = r1 + r3, t2i = i1 + i3;
  const float t3r = r1 - r3, t3i = i1 - i3;
  r0 = t0r + t2r; i0 = t0i + t2i;
  r2 = t0r - t2r; i2 = t0i - t2i;
  r1 = t1r + t3i; i1 = t1i - t3r;     // t1 - i*t3
  r3 = t1r - t3i; i3 = t1i + t3r;     // t1 + i*t3
}

// the same with a3 = 0 as a literal: the compiler folds x - 0 but not x + 0 (the sign of a zero), so the general form carries two
// additions of zero. Without them only the sign of an exact zero inside the transform can differ, and every output of the
// transform is squared before it is used (pk, pm, p128)
__device__ __forceinline__ void dft4_z3(float &r0, float &i0, float &r1, float &i1, float &r2, float &i2,
                                        float &r3, float &i3) {
  const float t0r = r0 + r2, t0i = i0 + i2;
  const float t1r = r0 - r2, t1i = i0 - i2;
  const float t2r = r1, t2i = i1;
  r0 = t0r + t2r; i0 = t0i + t2i;
  r2 = t0r - t2r; i2 = t0i - t2i;
  r1 = t1r + t2i; i1 = t1i - t2r;
  r3 = t1r - t2i; i3 = t1i + t2r;
}

__device__ __forceinline__ void cmul(float &r, float &i, float c, float s) {   // (r+ii)*(c+is)
  const float nr = fmaf(r, c, -i * s);
  const float ni = fmaf(r, s, i * c);
  r = nr; i = ni;
}
// the same with -s handed in as a value of its own: i * (-s) = -(i * s) exactly, and the product needs no negated operand
// (which only the 64-bit VOP3 form has)
__device__ __forceinline__ void cmul_ns(float &r, float &i, float c, float s, float ns) {
  const float nr = fmaf(r, c, i * ns);
  const float ni = fmaf(r, s, i * c);
  r = nr; i = ni;
}

// The constants of a DFT16 as wave-uniform register values (SGPRs): a literal makes a VOP2 instruction 64 bits long, and the
// 64-bit encoded forms issue every ~4.2 cycles where the 32-bit ones take ~2.8 (profiles/r06_valu_classes.json). The negatives
// are constants of their own: a negated operand would need the (64-bit) VOP3 form.
struct Dft16K {
  float c1, s1, r2, nc1, ns1, nr2;
  __device__ __forceinline__ Dft16K() : c1(C1), s1(S1), r2(R2), nc1(-C1), ns1(-S1), nr2(-R2) {
    asm volatile("" : "+s"(c1), "+s"(s1), "+s"(r2), "+s"(nc1), "+s"(ns1), "+s"(nr2));
  }
};

// forward DFT16, natural order in and out (registers, static indexing only).
// x[m], m = m0 + 4 m1:  y[m0][q] = DFT4 over m1; y *= w16^(m0 q);
// X[q + 4p] = DFT4 over m0.
// In three parts, so that the caller can put LDS traffic between them (round 8): dft16_first + dft16_last(q = 0 .. 3) + dft16_rename
// is dft16 -- one implementation of the arithmetic.
// first layer, group m0: needs the inputs m0, m0 + 4, m0 + 8, m0 + 12 only
// Z3: the input m0 + 12 is a literal zero (the sample pairs m >= MP of a frame that has fewer than sixteen per lane)
template <bool Z3 = false>
__device__ __forceinline__ void dft16_first(float (&re)[16], float (&im)[16], int m0) {
  if constexpr (Z3) dft4_z3(re[m0], im[m0], re[m0 + 4], im[m0 + 4], re[m0 + 8], im[m0 + 8], re[m0 + 12], im[m0 + 12]);
  else dft4(re[m0], im[m0], re[m0 + 4], im[m0 + 4], re[m0 + 8], im[m0 + 8], re[m0 + 12], im[m0 + 12]);
}
// y[m0][q] sits at index m0 + 4q. Twiddles w16^(m0*q), w16 = e^{-2 pi i/16}:
// (1,1)->e1 (1,2)->e2 (1,3)->e3 (2,1)->e2 (2,2)->e4 (2,3)->e6 (3,1)->e3 (3,2)->e6 (3,3)->e9
__device__ __forceinline__ void dft16_twiddles(float (&re)[16], float (&im)[16], const Dft16K &K) {
  cmul_ns(re[1 + 4], im[1 + 4], K.c1, K.ns1, K.s1);                       // e1
  { const float a = re[1 + 8], b = im[1 + 8]; re[1 + 8] = K.r2 * (a + b); im[1 + 8] = K.r2 * (b - a); }    // e2
  cmul_ns(re[1 + 12], im[1 + 12], K.s1, K.nc1, K.c1);                     // e3
  { const float a = re[2 + 4], b = im[2 + 4]; re[2 + 4] = K.r2 * (a + b); im[2 + 4] = K.r2 * (b - a); }    // e2
  { const float a = re[2 + 8], b = im[2 + 8]; re[2 + 8] = b; im[2 + 8] = -a; }                             // e4 = -i
  { const float a = re[2 + 12], b = im[2 + 12]; re[2 + 12] = K.r2 * (b - a); im[2 + 12] = K.nr2 * (a + b); }  // e6
  cmul_ns(re[3 + 4], im[3 + 4], K.s1, K.nc1, K.c1);                       // e3
  { const float a = re[3 + 8], b = im[3 + 8]; re[3 + 8] = K.r2 * (b - a); im[3 + 8] = K.nr2 * (a + b); }   // e6
  cmul_ns(re[3 + 12], im[3 + 12], K.nc1, K.s1, K.ns1);                    // e9
}
// last layer, group q: leaves the final X[q + 4p] at index 4q + p
__device__ __forceinline__ void dft16_last(float (&re)[16], float (&im)[16], int q) {
  dft4(re[4 * q], im[4 * q], re[4 * q + 1], im[4 * q + 1], re[4 * q + 2], im[4 * q + 2], re[4 * q + 3], im[4 * q + 3]);
}
// X[q + 4p] sits at index 4q + p: undo the digit reversal (register renaming)
__device__ __forceinline__ void dft16_rename(float (&re)[16], float (&im)[16]) {
  float tr[16], ti[16];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int p = 0; p < 4; ++p) { tr[q + 4 * p] = re[4 * q + p]; ti[q + 4 * p] = im[4 * q + p]; }
#pragma unroll
  for (int k = 0; k < 16; ++k) { re[k] = tr[k]; im[k] = ti[k]; }
}
__device__ __forceinline__ void dft16(float (&re)[16], float (&im)[16], const Dft16K &K) {
#pragma unroll
  for (int m0 = 0; m0 < 4; ++m0) dft16_first(re, im, m0);
  dft16_twiddles(re, im, K);
#pragma unroll
  for (int q = 0; q < 4; ++q) dft16_last(re, im, q);
  dft16_rename(re, im);
}

// DPP move with a compile-time control word (row_shl:n = 0x100 + n, row_ror:n = 0x120 + n, row_mirror = 0x140)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// The untangle partner's half of Z, in place on x[8 .. 15] and y[8 .. 15] (re and im of the second DFT16's outputs; lane-to-column
// map 0 .. 7, 9 .. 15, 8): lanes 1 .. 14 of every row take the register of the lane opposite (row_mirror), lane 15 keeps its own, lane 0
// moves its own x[r + 1] to x[r] for r = 8 .. 14 (x[15] stays: its q = 0 is the DC / Nyquist pair). Written out, because the compiler
// resolves the join of the three lane classes with 30 to 60 register-shuffling moves: here it is 16 DPP moves + 14 moves, and seven
// scalar moves of EXEC around them (saved and restored: the block leaves EXEC as it found it).
// Wait states: a DPP move reads a VGPR that a vector instruction may have written right in front of the block -- two wait
// states, which the three scalar moves in front of the first DPP move are; the DPP moves read and write disjoint registers; the plain
// moves behind them are interlocked by the hardware. A SCALAR write of EXEC needs no wait state in front of a DPP move (only a
// vector instruction's write of EXEC does).
__device__ __forceinline__ void untangle_partner(float (&x)[16], float (&y)[16]) {
  unsigned long long sv;
  asm volatile(
      "s_mov_b64 %[sv], exec\n"
      "s_mov_b32 exec_lo, 0x7ffe7ffe\n"
      "s_mov_b32 exec_hi, 0x7ffe7ffe\n"
      "v_mov_b32_dpp %[x8], %[x8] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[x9], %[x9] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[x10], %[x10] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[x11], %[x11] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[x12], %[x12] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[x13], %[x13] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[x14], %[x14] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[x15], %[x15] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[y8], %[y8] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[y9], %[y9] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[y10], %[y10] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[y11], %[y11] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[y12], %[y12] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[y13], %[y13] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[y14], %[y14] row_mirror row_mask:0xf bank_mask:0xf\n"
      "v_mov_b32_dpp %[y15], %[y15] row_mirror row_mask:0xf bank_mask:0xf\n"
      "s_mov_b32 exec_lo, 0x00010001\n"
      "s_mov_b32 exec_hi, 0x00010001\n"
      "v_mov_b32 %[x8], %[x9]\n"
      "v_mov_b32 %[x9], %[x10]\n"
      "v_mov_b32 %[x10], %[x11]\n"
      "v_mov_b32 %[x11], %[x12]\n"
      "v_mov_b32 %[x12], %[x13]\n"
      "v_mov_b32 %[x13], %[x14]\n"
      "v_mov_b32 %[x14], %[x15]\n"
      "v_mov_b32 %[y8], %[y9]\n"
      "v_mov_b32 %[y9], %[y10]\n"
      "v_mov_b32 %[y10], %[y11]\n"
      "v_mov_b32 %[y11], %[y12]\n"
      "v_mov_b32 %[y12], %[y13]\n"
      "v_mov_b32 %[y13], %[y14]\n"
      "v_mov_b32 %[y14], %[y15]\n"
      "s_mov_b64 exec, %[sv]\n"
      : [sv] "=&s"(sv), [x8] "+v"(x[8]), [x9] "+v"(x[9]), [x10] "+v"(x[10]), [x11] "+v"(x[11]), [x12] "+v"(x[12]), [x13] "+v"(x[13]), [x14] "+v"(x[14]), [x15] "+v"(x[15]), [y8] "+v"(y[8]), [y9] "+v"(y[9]), [y10] "+v"(y[10]), [y11] "+v"(y[11]), [y12] "+v"(y[12]), [y13] "+v"(y[13]), [y14] "+v"(y[14]), [y15] "+v"(y[15]));
}

}  // namespace

// The next pass's samples of one lane: pair n = j + 16 m of frame tp + g for m < MP. ALIGNED (the buffer is 4-byte
// aligned and every utterance starts at an even sample, checked on the host): one load per pair; otherwise two
// 16-bit loads (typed, i.e. converted to float by the buffer unit, or integer: typed_loads() below). `base` = first
// sample of the pass's first frame minus the left padding; the per-lane byte
// offset (g H + 2 j) * 2 is ONE VGPR and load m adds the immediate 64 m -- everything else is wave-uniform and lives in
// SGPRs: nothing to spill (a spill reload would put an s_waitcnt vmcnt(0) behind the loads and wait out the whole memory
// latency in every pass). Samples outside a frame meet a zero of the window table and every stored frame lies inside
// its utterance, so an out-of-range address needs no care: the buffer unit's range check answers it with zero (pcm_prefetch).
//
// PREEMPH: the predecessor x[2n - 1] of pair n's even sample is the neighbour lane's odd sample (DPP row_ror:1; lane 0 takes lane
// 15's of the register one pair down): no further vector-memory instruction.
//
// The conversion int16 -> float is the buffer unit's: a TYPED buffer load returns (float)x exactly. Aligned
// input: one tbuffer_load_format_xy [16_16, SSCALED] per pair in place of a dword load and two conversions; unaligned
// input: two tbuffer_load_format_x [16, SSCALED] in place of two 16-bit loads and two conversions. The number of
// vector-memory instructions is the integer form's, 2 MP vector instructions per pass are gone, and every later operation
// sees the same operands: the bits are the integer form's (tests/test_gpu_mfcc512_typed_loads.py). The loads are reached
// through the LLVM intrinsic by name -- no inline assembly: the compiler keeps its own s_waitcnt vmcnt bookkeeping and
// folds 64 m into the immediate offset.
// The samples are the window stage's own operands, so they have to DIE there: the pass loop sets them to zero on
// the path that issues no further prefetch (the wave's last pass). While they stayed alive on that path the
// pre-emphasis products could not overwrite their addend (v_fma_f32, 64-bit, instead of v_fmac) and 2 MP registers
// stayed occupied through both transforms.
// Per instance: the two floats per pair live from the prefetch issue to the window (aligned input: 2 MP registers
// where the dword form holds MP), and an instance whose scratch would grow against the dword form keeps that form
// (integer loads, v_cvt_f32_i32 on the vector ALU): the PLP chain (every instance of it stands at 128 VGPRs already) and
// the delta-fused instances with MP = 16. With this rule no instance has more scratch than with integer loads, all have
// <= 128 VGPRs and occupancy 4
// (tools/dev/kernel_resources.sh lld_mfcc512.hip).
template <int MP, bool PLP, bool DELTA>
constexpr bool typed_loads() {
  return !PLP && !(MP == 16 && DELTA);
}
// The untangle partner by the column map and one row_mirror (untangle_partner above) or, without the map, in three DPP steps.
// Per instance: the one-hop form holds the lane's column and bin 128's value (taken in front of the exchange) in two registers
// more at the point where the instances at 128 VGPRs are full -- with it the 21 instances of the PLP chain and of MP = 16 with the
// regression stages fused had 4 or 8 bytes more scratch per lane each. They keep the three-step form: the rule is typed_loads()'s,
// and with it no instance has more scratch than before (tools/dev/kernel_resources.sh lld_mfcc512.hip).
template <int MP, bool PLP, bool DELTA>
constexpr bool one_hop_exchange() {
  return !PLP && !(MP == 16 && DELTA);
}
// The transposition through the split-complex buffer (tsplit_base above) with address-free stores, or through the interleaved
// buffer of (re, im) pairs with ds_write_b64 / ds_read_b64. Per instance: the split form is taken by the instances of the bench's
// class -- the column map of one_hop_exchange(), the same rule -- which is the class it was timed in (DESIGN 4.1,
// profiles/split_transpose_ab.txt). The PLP chain and the delta-fused MP = 16 instances keep the interleaved buffer: nobody has
// timed them. Statically the split form would suit them as well (the row table serves kc = j too; compiled for all 108 instances
// no instance had more scratch -- 1524 -> 992 bytes per lane summed over the 32 that have any --, all had <= 128 VGPRs, occupancy
// >= 4 and two blocks per CU: tools/dev/kernel_resources.sh lld_mfcc512.hip) and their bits were the parent's.
template <int MP, bool PLP, bool DELTA>
constexpr bool split_transpose() {
  return !PLP && !(MP == 16 && DELTA);
}
// One index k1 of the first DFT16 into its two rows: the wave's region is M0 (set at the head of the pass), the row an immediate.
// (The compiler does not count these stores in its s_waitcnt lgkmcnt bookkeeping: a wait of its own then stands for MORE
// outstanding operations than it counted and returns later, never earlier; LDS operations of a wave complete in order.)
template <int K1>
__device__ __forceinline__ void tsplit_store(float x, float y) {
  asm volatile("ds_write_addtid_b32 %0 offset:%2\n\tds_write_addtid_b32 %1 offset:%3"
               :
               : "v"(x), "v"(y), "i"(4 * tsplit_base(K1, false)), "i"(4 * tsplit_base(K1, true))
               : "memory");
}
__device__ __forceinline__ void tsplit_store_k1(int k1, float x, float y) {   // k1 is a constant after unrolling
  switch (k1) {
#define SMILEHIP_TSPLIT_CASE(K) case K: tsplit_store<K>(x, y); break;
    SMILEHIP_TSPLIT_CASE(0) SMILEHIP_TSPLIT_CASE(1) SMILEHIP_TSPLIT_CASE(2) SMILEHIP_TSPLIT_CASE(3)
    SMILEHIP_TSPLIT_CASE(4) SMILEHIP_TSPLIT_CASE(5) SMILEHIP_TSPLIT_CASE(6) SMILEHIP_TSPLIT_CASE(7)
    SMILEHIP_TSPLIT_CASE(8) SMILEHIP_TSPLIT_CASE(9) SMILEHIP_TSPLIT_CASE(10) SMILEHIP_TSPLIT_CASE(11)
    SMILEHIP_TSPLIT_CASE(12) SMILEHIP_TSPLIT_CASE(13) SMILEHIP_TSPLIT_CASE(14) SMILEHIP_TSPLIT_CASE(15)
#undef SMILEHIP_TSPLIT_CASE
    default: break;
  }
}
typedef float float4v __attribute__((ext_vector_type(4)));
typedef float float2v __attribute__((ext_vector_type(2)));
__device__ float2v tbuffer_load_xy(__amdgpu_buffer_rsrc_t rsrc, int voffset, int soffset, int format, int aux)
    __asm("llvm.amdgcn.raw.ptr.tbuffer.load.v2f32");
__device__ float tbuffer_load_x(__amdgpu_buffer_rsrc_t rsrc, int voffset, int soffset, int format, int aux)
    __asm("llvm.amdgcn.raw.ptr.tbuffer.load.f32");
// gfx9 MTBUF encoding: dfmt | nfmt << 4 with dfmt BUF_DATA_FORMAT_16_16 = 5, BUF_DATA_FORMAT_16 = 2 and
// nfmt BUF_NUM_FORMAT_SSCALED = 3
constexpr int kFmt16x2Sscaled = 5 | (3 << 4);
constexpr int kFmt16Sscaled = 2 | (3 << 4);
// word 3 of the descriptor: DATA_FORMAT_32 (bits 18:15; what the untyped loads always had) and, for the typed loads,
// DST_SEL_X = 4 (the element's first component), DST_SEL_Y = 5 (its second) in bits 5:0 -- a selector of 0 returns the
// constant zero; untyped loads ignore the field
constexpr int kRsrcWord3 = 0x00020000, kRsrcWord3Typed = 0x00020000 | 4 | (5 << 3);

// TYPED: v holds the two floats of pair m (their bits) in v[2 m], v[2 m + 1]; integer loads: pair m as one dword in v[m]
// (ALIGNED) or its two sign-extended samples in v[2 m], v[2 m + 1]
template <int MP, bool ALIGNED, bool TYPED>
struct FrameRegs {
  uint32_t v[ALIGNED && !TYPED ? MP : 2 * MP];
};

// The loads are BUFFER loads: a wave-uniform resource descriptor (base = the pass's first sample, size = what is left of the
// PCM buffer behind it) in four SGPRs, ONE VGPR of per-lane byte offset and the immediate 64 m -- no 64-bit address arithmetic on the
// vector ALU (global loads spent 13 v_lshl_add_u64 and 26 address VGPRs per pass on it), and the hardware's range check
// replaces a clamped-address branch: a read behind the end of the buffer (or in front of it: the offset wraps to a huge unsigned
// value) returns zero, which is as good as the clamped sample -- such samples meet a zero of the window table or belong to a frame
// that is not stored.
template <int MP, bool ALIGNED, bool TYPED>
__device__ __forceinline__ void pcm_prefetch(const int16_t *pcm, int64_t pcm_total, int64_t base, int H, int lane,
                                             FrameRegs<MP, ALIGNED, TYPED> &R) {
  const int64_t b0 = base < 0 ? 0 : base;                // (negative only for the buffer's first frames under symmetric zero padding)
  int64_t left = (pcm_total - b0) * 2;                   // bytes behind the descriptor's base
  left = left < 0 ? 0 : (left > 0xfffffffcLL ? 0xfffffffcLL : left);
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<int16_t *>(pcm + b0), 0, (int)(uint32_t)left,
                                                                        TYPED ? kRsrcWord3Typed : kRsrcWord3);
  uint32_t lo = ((uint32_t)(lane >> 4) * (uint32_t)H + 2u * (uint32_t)(lane & 15)) * 2u + (uint32_t)((base - b0) * 2);
  asm volatile("" : "+v"(lo));                           // opaque per call: no hoisted per-m offset registers
#pragma unroll
  for (int m = 0; m < MP; ++m) {
    if constexpr (TYPED && ALIGNED) {
      const float2v f = tbuffer_load_xy(rsrc, (int)lo + 64 * m, 0, kFmt16x2Sscaled, 0);
      R.v[2 * m] = __float_as_uint(f.x);
      R.v[2 * m + 1] = __float_as_uint(f.y);
    } else if constexpr (TYPED) {
      R.v[2 * m] = __float_as_uint(tbuffer_load_x(rsrc, (int)lo + 64 * m, 0, kFmt16Sscaled, 0));
      R.v[2 * m + 1] = __float_as_uint(tbuffer_load_x(rsrc, (int)lo + 64 * m + 2, 0, kFmt16Sscaled, 0));
    } else if constexpr (ALIGNED) {
      R.v[m] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)lo + 64 * m, 0, 0);
    } else {
      R.v[2 * m] = (uint32_t)(int32_t)(int16_t)__builtin_amdgcn_raw_buffer_load_b16(rsrc, (int)lo + 64 * m, 0, 0);
      R.v[2 * m + 1] = (uint32_t)(int32_t)(int16_t)__builtin_amdgcn_raw_buffer_load_b16(rsrc, (int)lo + 64 * m + 2, 0, 0);
    }
  }
}

// the phases of the pass loop (phase_timing.hpp; tools/ubench/variant.sh phase -DSMILEHIP_PHASE_TIMING, tools/ubench/phase_timing.py)
SMILEHIP_PHASE_COUNTERS(g_phase, 16, smilehip_debug_phase)
// every wave's lifetime in the pass loop and where it ran (wave_lifetimes.hpp; tools/ubench/variant.sh lifetimes -DSMILEHIP_PHASE_TIMING=2,
// tools/ubench/wave_lifetimes.py)
SMILEHIP_WAVE_LIFE_RECORDS(g_wave_life, smilehip_debug_wave_life)

// Issue priority of the wave, level & 3 (wave-uniform): s_setprio takes an immediate, hence a scalar branch -- no vector instruction.
// The pass loop rotates it: a SIMD arbitrates vector issue by priority, then by AGE, the loop has no barrier and gives every
// wave the same work, so at equal priority the age order of a SIMD's four waves held for the whole launch -- the oldest ran at
// nearly single-wave speed and left first, the SIMD ended the launch with three, two, one wave (lifetimes 0.59 / 0.68 / 0.82 /
// 0.96 of the longest by start order, finish order = start order on 1023 of 1024 SIMDs: profiles/wave_lifetimes_parent.json).
// With level = passes done + the wave's slot on its SIMD, the four waves of a SIMD hold four different levels in every pass and
// each level for a quarter of its passes; a wave that runs ahead hurries through its high passes and lingers in its low ones,
// so no wave needs to know another's progress. Lifetimes 0.86 / 0.88 / 0.93 / 0.96, resident waves per SIMD 2.97 -> 3.52 of the
// pass loop (profiles/wave_lifetimes.json), the bench step -3.7 % and -4.6 % in two visits (profiles/wave_order_ab.txt).
__device__ __forceinline__ void wave_set_prio(int level) {
  switch (level & 3) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
  }
}

// LDS layout (dynamic), sizes in floats:
//   shared tables : tw512 [256 f2] | win [MP*16 f2] | tw256 [256 f2, index k1*16+j] |
//                   melw0 [UC*16 f4] | melw1 [UC*16 f4] | dct [16 x 28] | plp [48]
//   per wave      : 4 x (log-mel [32] | acf [16] | cepstra [16]) | 4 x power buffer [448];
//                   the transpose buffer (split-complex [2092]; interleaved (re,im) pairs [2078]) overlays all of it between the
//                   two DFT16. With the split-complex buffer the eight per-wave regions stand in FRONT of the shared tables
// DELTA: the two regression stages behind the static coefficients (cDeltaRegression, deltaRegression.cpp:144-152, deltawin = 2,
// twice) computed by the same waves -- a lane keeps its coefficient of the previous pass's frame and the two passes' first-order
// values in registers, takes its neighbours' through the LDS crossbar (ds_bpermute: no storage), and writes static | delta |
// acceleration cells of the final rows. The expressions and the index clamps are lld_chain_tiled's (lld_kernels.hip: chain_op,
// level 1 has T + 2 rows, all of which level 2 reads as data), so the values equal the separate kernel's bit for bit
// (tests/test_gpu_mfcc.py::test_fused_delta_equals_window_chain). Tiles are FTileRec (lld_params.hpp).
// PAD0 (round 7): the frame's first sample is pair 0's even sample (pad_left = 0: every geometry without zeroPadSymmetric), so
// R2's first-sample fix-up y[0] = (1-k) x[0] is one select at m = 0 instead of one per m (the general form's sample position is
// a runtime value). The kernels lld_mfcc512 (PAD0, and every instance without pre-emphasis) and lld_mfcc512_padded (any pad_left,
// instantiated with PREEMPH only) below share this body.
template <int MP, bool PREEMPH, bool USE_POWER, bool ALIGNED, bool PLP, int UC, bool DELTA, bool PAD0>
__device__ __forceinline__ void lld_mfcc512_body(const LldParams &P, const Fast512Tables &F) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63;
  // wave-uniform by construction; tell the compiler so that everything derived from it
  // (tile, utterance, offsets, pointers) lives in SGPRs instead of VGPR pairs
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4;
  const int j = lane & 15;

  // ---- carve shared memory (split-complex transposition: the per-wave regions first, see kTSWaveFloats)
  constexpr bool kOneHop = one_hop_exchange<MP, PLP, DELTA>();
  constexpr bool kSplit = split_transpose<MP, PLP, DELTA>();
  constexpr int kWaveRegion = kSplit ? kTSWaveFloats : kWaveFloats;
  typedef __attribute__((address_space(3))) float *LdsFloatPtr;
  float *tables = smem;
  if constexpr (kSplit) {
    // behind 65 KB of wave regions no table offset fits an LDS instruction's 16-bit immediate: the tables' base is an opaque
    // scalar, so that the compiler adds it to the per-lane part of an address once and keeps the small immediates it always had
    // (with the constant in sight it built one address register per offset and spilled them)
    uint32_t tb = (uint32_t)(uintptr_t)(LdsFloatPtr)smem + 4u * kWavesPerBlock * kWaveRegion;
    asm volatile("" : "+s"(tb));
    tables = (float *)(LdsFloatPtr)(uintptr_t)tb;
  }
  float2 *s_tw512 = reinterpret_cast<float2 *>(tables);
  float2 *s_win = s_tw512 + 256;
  float2 *s_tw256 = s_win + MP * 16;
  float4 *s_melw0 = reinterpret_cast<float4 *>(s_tw256 + 256);
  float4 *s_melw1 = s_melw0 + UC * 16;
  float *s_dct = reinterpret_cast<float *>(s_melw1 + UC * 16);
  float *s_plp = s_dct + 16 * 28;                                    // PLP chain: eql[32] | sintable[16]
  constexpr int shared_floats = 256 * 2 + MP * 16 * 2 + 256 * 2 + UC * 16 * 8 + 16 * 28 + 48;
  float *wbase = smem + (kSplit ? 0 : shared_floats) + wave * kWaveRegion;
  float *s_lmel = wbase + g * kLmelFloats;                        // log-mel of my frame (28 read by the DCT)
  float *s_cep = s_lmel + 48;                                     // PLP: 16 cepstra behind the band vector and its 16 acf lags
  float *s_pb = wbase + 4 * kLmelFloats + g * kPbFloats;          // power spectrum of my frame

  // ---- cooperative load of the shared tables
  for (int i = threadIdx.x; i < 256; i += blockDim.x) { s_tw512[i] = F.tw512[i]; s_tw256[i] = F.tw256[i]; }
  for (int i = threadIdx.x; i < MP * 16; i += blockDim.x) s_win[i] = F.win[i];
  for (int i = threadIdx.x; i < UC * 16; i += blockDim.x) { s_melw0[i] = F.melw[2 * i]; s_melw1[i] = F.melw[2 * i + 1]; }
  for (int i = threadIdx.x; i < 16 * 28; i += blockDim.x) s_dct[i] = F.dct28[i];
  if (PLP) {
    for (int i = threadIdx.x; i < 32; i += blockDim.x) s_plp[i] = F.plp_eql[i];
    for (int i = threadIdx.x; i < 16; i += blockDim.x) s_plp[32 + i] = F.plp_sin[i];
  }
  __syncthreads();

  uint32_t mo[UC];                              // byte offsets of my units' octets in the power buffer
#pragma unroll
  for (int i = 0; i < UC; ++i) mo[i] = F.melo[i * 16 + j];
  // which of my units belong to my first band (bit i) | first band << 8 | second band << 16 (0xff: none)
  const uint32_t lane_bands = (uint32_t)F.lane_bands[j];
  const int band0 = (int)((lane_bands >> 8) & 0xffu), band1 = (int)((lane_bands >> 16) & 0xffu);
  // 1.0f / 0.0f per unit: the unit's sum goes to the lane's first / second band as a0 = fma(acc, uf0, a0), a1 = fma(acc, uf1, a1) --
  // acc x 1 is exact and acc x 0 = 0 (the sums are finite and >= 0), so the two band sums are the ones a select + add produced, bit
  // for bit, for two 32-bit encoded v_fmac instead of two selects (64-bit encoded, a lane mask in an SGPR pair each) + two adds
  float uf0[UC], uf1[UC];
#pragma unroll
  for (int i = 0; i < UC; ++i) { uf0[i] = ((lane_bands >> i) & 1u) ? 1.0f : 0.0f; uf1[i] = 1.0f - uf0[i]; }
  // my cell relative to the pass's base row: the row of the pass's first frame -- DELTA: of the frame four before it, whose
  // static | delta | acceleration cells a pass writes together (whole rows: 4 x 156 consecutive bytes per wave and pass.
  // Writing each value as soon as it exists -- three stores into three different sets of rows -- cost 0.05 ms per 998 000 frames)
  const uint32_t out_off = (uint32_t)(g * (int)P.ld_out + j) * 4u;
  const uint32_t out_off_d = out_off + (uint32_t)P.n_mfcc * 4u;
  const uint32_t out_off_dd = out_off + (uint32_t)P.n_mfcc * 8u;
  const float nkpre = P.de ? P.k : -P.k;       // y = x + nkpre * x'  (de: y = x + k x'), wave-uniform: the FMAs below stay v_fmac
  const int m0 = P.pad_left >> 5, j0 = (P.pad_left >> 1) & 15;       // where sample 0 of a frame sits
  // The column of the second DFT16 that lane j transforms: 0 .. 7, 9 .. 15, 8 (one_hop_exchange()) -- the lane's bins, their
  // twiddles and their places in the power buffer go by kc; everything in front of the transposition's loads and behind the power
  // buffer goes by j. kc(0) = 0: lane 0 stays the lane of DC / Nyquist and of bin 128.
  const int kc = !kOneHop ? j : (j < 8 ? j : (j == 15 ? 8 : j + 1));
  // split-complex transposition: the wave's region as the stores' M0 (an LDS byte address) and the reader's one address -- columns
  // 0 .. 15 of row kc of my group in the real plane, the imaginary plane 128 floats behind it
  const uint32_t wbase_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(LdsFloatPtr)wbase);
  int ts_row = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (kc == r) ts_row = tsplit_base(r, false);
  const float *ts_rd = wbase + ts_row + 16 * g;
  float *pb_k = s_pb + pb_pos(kc);             // my bins k = kc + 16 q sit 24 q floats further on
  float *pb_m = s_pb + pb_pos(256 - kc);       // their mirror images 256 - k sit 24 q floats back

  const Dft16K dk;
  PhaseTimer<12> PH;
  // Persistent waves walk tiles tile, tile + #waves, ... as ONE flat stream of passes: the
  // next pass's PCM (same tile or the first pass of the next tile) is always in flight, tile
  // records are fetched one tile ahead, and a pass's results are stored at the top of the
  // following pass. The only s_waitcnt vmcnt in steady state is the one that consumes the
  // prefetched PCM, and everything older than those loads was issued a full pass earlier.
  const int tile_stride = __builtin_amdgcn_readfirstlane((int)gridDim.x) * kWavesPerBlock;   // (a vector load otherwise)
  int tile = blockIdx.x * kWavesPerBlock + wave;
  const int n_tiles = DELTA ? P.n_ftiles : P.n_tiles;
  if (tile >= n_tiles) return;                         // wave-uniform; no block barrier below
  // records are read through the constant address space: read-only for the kernel's lifetime,
  // so wave-uniform addresses become s_load and the values (and every address derived from
  // them) stay in SGPRs
  typedef typename std::conditional<DELTA, FTileRec, TileRec>::type Rec;
  typedef const __attribute__((address_space(4))) Rec *ConstRecPtr;
  const ConstRecPtr recs = DELTA ? (ConstRecPtr)(uintptr_t)P.ftile_rec : (ConstRecPtr)(uintptr_t)P.tile_rec;
  int64_t cur_samp0 = recs[tile].samp0, cur_row0 = recs[tile].row0;
  int cur_n = recs[tile].n_frames;
  // DELTA: frames behind the utterance's end | rows this tile writes | the utterance's first frame | regression stages on
  int cur_live = 0, cur_e0 = 0, cur_e1 = 0, cur_lo = 0, cur_don = 0;
  if constexpr (DELTA) {
    cur_live = recs[tile].live_n; cur_e0 = recs[tile].e0; cur_e1 = recs[tile].e1; cur_lo = recs[tile].lo; cur_don = recs[tile].delta_on;
  }
  // of the next tile's record only the first sample is held ahead (the prefetch of its first pass needs it a pass early); the
  // other fields are read when the wave moves on to the tile -- an s_load once per eight passes instead of ten SGPRs across the loop
  bool has_next = tile + tile_stride < n_tiles;
  int64_t nxt_samp0 = cur_samp0;
  if (has_next) nxt_samp0 = recs[tile + tile_stride].samp0;
  int tp = 0;                                          // first frame of the pass, relative to the tile
  constexpr bool TYPED = typed_loads<MP, PLP, DELTA>();
  FrameRegs<MP, ALIGNED, TYPED> R;
  pcm_prefetch<MP, ALIGNED, TYPED>(P.pcm, P.pcm_total, cur_samp0 - P.pad_left, P.H, lane, R);
  unsigned char *pend_row = nullptr;                   // deferred store of the previous pass (wave-uniform row base)
  float pend_val = 0.0f;
  bool pend_live = false;
  // DELTA: the previous pass's coefficient (frame tp - 4 + g), this and the previous pass's first-order values (frames
  // tp - 2 + g, tp - 6 + g); the deferred delta / acceleration cells
  float s_prev = 0.0f, d_cur = 0.0f;
  // ... and what the regression stage of the pass that has just ended works on: that pass's tile constants
  int b_tp = 0, b_lo = 0, b_live = 0, b_e0 = 0, b_e1 = 0, b_don = 0;
  // The regression stages of one pass: s_cur = the pass's coefficients (frame btp + g), s_prev the previous pass's, dp the previous
  // pass's first-order values (frame btp - 6 + g). Level 0 is held for the relative frames btp - 4 .. btp + 3 (s_prev of group
  // f & 3 for f < btp, s_cur behind it), level 1 for btp - 6 .. btp + 1 (dp / dn of group (f - (btp - 2)) & 3). An index is clamped
  // to its level's rows first: [lo, live_n - 1] for level 0, [lo, live_n + 1] for level 1 (T + deltawin rows, all of them data
  // for level 2). The expressions are chain_op's (lld_kernels.hip).
  const auto from_group = [&](int grp, float v) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(4 * ((grp << 4) | j), __float_as_int(v)));
  };
  const auto regress = [](float vm2, float vm1, float vp1, float vp2) {
    float num = 0.0f;
    num += 1.0f * (vp1 - vm1);
    num += 2.0f * (vp2 - vm2);
    return num;
  };
  // straight-line form for a pass none of whose indices is clamped: own registers and the two neighbour groups; the quotient by
  // Markstein's sequence (div_markstein, lld_device.hpp; tests/test_gpu_device_math.py checks the divisor 10 on the device). `plain`: a numerator
  // outside the range the sequence is safe for (zero keeps its sign only under the division) -> the pass takes delta_exact.
  const auto div10 = [](float a, bool &plain) {
    const float y = 0.1f, b = 10.0f;              // y = RN(1 / 10); norm = 2 (1 + 4), deltaRegression.cpp:77-79
    plain |= div_needs_division(a);
    return div_markstein(a, b, y);
  };
  const auto delta_fast = [&](float s_cur, float dp, float &dn, float &ddn, float &drow, bool &plain) {
    const float s1 = from_group((g + 1) & 3, g == 0 ? s_cur : s_prev);     // (the SOURCE lane chooses: group 0 holds frame btp, the others btp - 3 ..)
    const float s3 = from_group((g + 3) & 3, g == 3 ? s_prev : s_cur);
    dn = div10(regress(s_prev, s1, s3, s_cur), plain);                     // frame btp - 2 + g
    const float d1 = from_group((g + 1) & 3, g == 0 ? dn : dp);
    const float d3 = from_group((g + 3) & 3, g == 3 ? dp : dn);
    ddn = div10(regress(dp, d1, d3, dn), plain);                           // frame btp - 4 + g
    drow = from_group((g + 2) & 3, g >= 2 ? dp : dn);                      // the first-order value of frame btp - 4 + g
  };
  // any pass: clamped indices, the division itself
  const auto delta_exact = [&](float s_cur, float dp, int btp, int lo, int live_n, float &dn, float &ddn, float &drow) {
    const auto fetch = [&](int x, int hi_c, int base, float cur, float prev) {   // index x of a level held from `base - 4` on
      x = x < lo ? lo : (x > hi_c ? hi_c : x);
      const int dd = x - base;                                                   // -4 .. 3
      const float c = from_group(dd & 3, cur), p = from_group(dd & 3, prev);
      return dd >= 0 ? c : p;
    };
    const float norm = 10.0f;
    const int fd = btp - 2 + g, fdd = btp - 4 + g, hi0 = live_n - 1, hi1 = live_n + 1;
    dn = regress(fetch(fd - 2, hi0, btp, s_cur, s_prev), fetch(fd - 1, hi0, btp, s_cur, s_prev), fetch(fd + 1, hi0, btp, s_cur, s_prev),
                 fetch(fd + 2, hi0, btp, s_cur, s_prev)) / norm;
    ddn = regress(fetch(fdd - 2, hi1, btp - 2, dn, dp), fetch(fdd - 1, hi1, btp - 2, dn, dp), fetch(fdd + 1, hi1, btp - 2, dn, dp),
                  fetch(fdd + 2, hi1, btp - 2, dn, dp)) / norm;
    drow = from_group((g + 2) & 3, g >= 2 ? dp : dn);
  };

  // the wave's slot on its SIMD (HW_REG_HW_ID, WAVE_ID): the four resident waves of a SIMD hold four different ones
  // (slots 0 .. 3 on every SIMD of the bench launch, two waves of each of the CU's two blocks: the lifetime record)
  const int slot = (int)(__builtin_amdgcn_s_getreg((3 << 11) | 4) & 3u);
  int passes_done = 0;                                 // never reset: runs on across tile changes (tp does not)
  WaveLife WL;
  WL.begin();
  for (;;) {
    wave_set_prio(passes_done + slot);
    passes_done += 1;
    // M0 for the pass's address-free stores: written here and nowhere else in the kernel (the compiler has no use for M0 in this
    // kernel: tests/test_mfcc512_split_transpose_static.py reads the assembly); one wait state between a scalar write of M0 and an
    // LDS instruction that adds the lane number to it
    if constexpr (kSplit) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" : : "s"(wbase_lds));
    const bool live = tp + g < (DELTA ? cur_live : cur_n);
    PH(0);                                   // loop overhead
    // ------------------------------------------------------------ frame from registers: R0 (scale folded), R2, R3
    if constexpr (!DELTA) {
      if (pend_row != nullptr && pend_live) {     // previous pass's coefficients
        uint32_t oo = out_off;
        asm volatile("" : "+v"(oo));             // keep the 32-bit offset, not a hoisted 64-bit pointer
        *reinterpret_cast<float *>(pend_row + oo) = pend_val;
      }
    }
    // DELTA: the regression stages of the pass that has just ended, in the same basic block as the window arithmetic below (their
    // five crossbar round trips hide behind it); a pass with a clamped index or an unsafe numerator is redone behind it
    float st_dn = 0.0f, st_ddn = 0.0f, st_drow = 0.0f;
    bool st_plain = false;
    if constexpr (DELTA) delta_fast(pend_val, d_cur, st_dn, st_ddn, st_drow, st_plain);
    float re[16], im[16];
    {
      float tprev = 0.0f;                        // odd sample of pair 15 + 16 (m-1), as lane j = 0 needs it
      (void)tprev;
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        if (m < MP) {
          float a, b;
          if constexpr (TYPED) {                   // converted by the buffer unit
            a = __uint_as_float(R.v[2 * m]);
            b = __uint_as_float(R.v[2 * m + 1]);
          } else if constexpr (ALIGNED) {
            a = (float)(int16_t)(R.v[m] & 0xffffu);
            b = (float)(int16_t)(R.v[m] >> 16);
          } else {
            a = (float)(int32_t)R.v[2 * m];
            b = (float)(int32_t)R.v[2 * m + 1];
          }
          float ya = a, yb = b;
          if (PREEMPH) {
            const float t = dpp_f<0x121>(b);       // row_ror:1 -- lane j sees the odd sample of pair j-1 (lane 0: of lane 15)
            const float pa = (j == 0) ? tprev : t;   // x[2n - 1]
            tprev = t;
            // One rounding where the reference has two (preemphasis.cpp: x - k x' as a product and a difference): 26 vector
            // instructions fewer per pass, 0.3745 -> 0.3665 ms per 998 000 frames, and the distance to the reference went DOWN
            // (per-frame-scaled 1.048e-6 -> 1.041e-6, max abs 1.56e-4 -> 1.49e-4: the fused form is the exact difference rounded once).
            // This kernel's contract is the 1e-5 gate; the reference's own rounding sequence is lld_mfcc_generic's.
            // yb first: then both are v_fmac (the addend is the destination, -k an SGPR operand), no VOP3 v_fma_f32.
            yb = fmaf(nkpre, a, b);
            ya = fmaf(nkpre, pa, a);
            if (PAD0 ? (m == 0 && j == 0) : (m == m0 && j == j0)) ya = P.one_minus_k * a;      // y[0] = (1-k) x[0]
          }
          const float2 w = s_win[m * 16 + j];
          re[m] = ya * w.x;
          im[m] = yb * w.y;
        } else {
          re[m] = 0.0f; im[m] = 0.0f;
        }
      }
    }
    PH(1);                                   // wait for the prefetch, pre-emphasis, window
    if constexpr (DELTA) {
      // (first pass of a wave: the tile constants are zero, nothing is written)
      const bool clamped = !(b_tp - 6 >= b_lo && b_tp + 3 <= b_live - 1);
      if (clamped || __builtin_amdgcn_ballot_w64(st_plain && j < P.n_mfcc) != 0) delta_exact(pend_val, d_cur, b_tp, b_lo, b_live, st_dn, st_ddn, st_drow);
      // The row of frame b_tp - 4 + g, complete (static | delta | acceleration: 4 x 156 consecutive bytes per wave and pass). The
      // stores stand BEHIND the consumption of the prefetched samples: in front of it the compiler waited for them too
      // (s_waitcnt vmcnt(0) -- the path on which no store was issued decides the count): a store round trip per pass.
      const int fdd = b_tp - 4 + g;
      const bool row_live = pend_row != nullptr && j < P.n_mfcc && fdd >= b_e0 && fdd < b_e1;
      if (row_live) {
        uint32_t oo = out_off;
        asm volatile("" : "+v"(oo));               // keep the 32-bit offset, not a hoisted 64-bit pointer
        *reinterpret_cast<float *>(pend_row + oo) = s_prev;
      }
      if (row_live && b_don) {
        uint32_t oo = out_off_d;
        asm volatile("" : "+v"(oo));
        *reinterpret_cast<float *>(pend_row + oo) = st_drow;
        oo = out_off_dd;
        asm volatile("" : "+v"(oo));
        *reinterpret_cast<float *>(pend_row + oo) = st_ddn;
      }
      s_prev = pend_val;
      d_cur = st_dn;
    }

    // ------------------------------------------------------------ 256-point complex FFT
    // 16x16 transpose of (re, im) pairs: 16 ds_write_b64 + 16 ds_read_b64 through a buffer that
    // overlays the whole per-wave region (band vector and power buffers are dead here).
    // Element (row r, column c) of group g sits at byte g*128 + r*520 + c*8: the four groups'
    // rows are interleaved and each 4-group row is padded by 8 bytes, which makes both the
    // row-wise b64 stores (16-lane groups) and the column-wise b64 loads (32-lane groups)
    // bank-conflict free with immediate offsets only (tools/lds_bank_sim.py).
    float2 *tbw = reinterpret_cast<float2 *>(wbase) + g * 16 + j;
    const float2 *tbr = reinterpret_cast<const float2 *>(wbase) + g * 16 + kc * kTB2Row;
    {
      // The last layer of the DFT hands out final values group by group -- q = 0 gives k1 = 0, 4, 8, 12 -- so the twiddle
      // product and the ds_write_b64 of an index follow its dft4 at once: the sixteen writes are spread over the last layer and the
      // twiddles instead of standing in one block in front of the reads (0.3808 -> 0.3756 ms per bench step). The twiddle pairs of
      // group q + 1 are requested before group q's last layer (those of group 0 before the whole DFT): no table read stands behind a
      // transposition write that the compiler cannot tell apart from it, and each has ~30 vector instructions to arrive in.
      float2 w[4], wn[4];
#pragma unroll
      for (int p = 1; p < 4; ++p) w[p] = s_tw256[(4 * p) * 16 + j];
      w[0] = make_float2(1.0f, 0.0f);              // k1 = 0: no product
#pragma unroll
      for (int m0 = 0; m0 < 4; ++m0) {
        if (m0 + 12 >= MP) dft16_first<true>(re, im, m0);      // MP = 13: m = 13, 14, 15 are literal zeros
        else dft16_first(re, im, m0);
      }
      dft16_twiddles(re, im, dk);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q < 3) {
#pragma unroll
          for (int p = 0; p < 4; ++p) wn[p] = s_tw256[(q + 1 + 4 * p) * 16 + j];
        }
        dft16_last(re, im, q);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int k1 = q + 4 * p;
          if (k1 > 0) cmul(re[4 * q + p], im[4 * q + p], w[p].x, w[p].y);
          if constexpr (kSplit) tsplit_store_k1(k1, re[4 * q + p], im[4 * q + p]);
          else tbw[k1 * kTB2Row] = make_float2(re[4 * q + p], im[4 * q + p]);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) w[p] = wn[p];
      }
    }
    PH(3);                                   // dft16 + twiddles (+ transposition writes)
    {
      wave_lds_fence();
      if constexpr (kSplit) {                    // four ds_read_b128 per plane: columns 4 i .. 4 i + 3 (4 LDS cycles each)
        typedef const volatile __attribute__((address_space(3))) float4v *LdsF4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float4v v = ((LdsF4)ts_rd)[i];
          re[4 * i] = v.x; re[4 * i + 1] = v.y; re[4 * i + 2] = v.z; re[4 * i + 3] = v.w;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float4v v = ((LdsF4)ts_rd)[32 + i];
          im[4 * i] = v.x; im[4 * i + 1] = v.y; im[4 * i + 2] = v.z; im[4 * i + 3] = v.w;
        }
      } else {
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {          // one ds_read_b64 each (2 LDS cycles); paired into ds_read2_b64 they would take 8 per pair
        typedef const volatile __attribute__((address_space(3))) unsigned long long *LdsU64;
        const unsigned long long v = ((LdsU64)tbr)[jj];
        re[jj] = __int_as_float((int)(uint32_t)v); im[jj] = __int_as_float((int)(uint32_t)(v >> 32));
      }
      }
      wave_lds_fence();
    }
    PH(4);                                   // transposes
    dft16(re, im, dk);                                       // over j -> k2 ; Z[j + 16 k2]
    PH(5);                                   // second dft16

    // ------------------------------------------------------------ untangle pairs + power
    // Bin kc + 16 q pairs with bin 256 - kc - 16 q = (16 - kc) + 16 (15 - q): column 16 - kc, register 15 - q. Under the column
    // map lanes 1 .. 14 hold columns i and 16 - i in lanes i and 15 - i, so ONE row_mirror per value is the exchange, in place on
    // re[8 .. 15] / im[8 .. 15] (the owner reads only its registers 0 .. 7 from here on). Lane 15 (column 8) is its own partner in the
    // same register and keeps what it has. Lane 0 (column 0) is its own partner one register up (bin 256 - 16 q = 0 + 16 (16 - q)):
    // seven plain moves per component with lane 0 of each row enabled alone; its q = 0 is the DC / Nyquist pair, handled below,
    // and its own re[8], im[8] make bin 128, taken before the shift.
    float p128 = 0.0f;
    if constexpr (kOneHop) {
      const float a = re[8], b = im[8];
      p128 = 4.0f * fmaf(b, b, a * a);
      untangle_partner(re, im);
    } else {
      // (the exchange in three dependent DPP steps: instances that hold their registers only so, one_hop_exchange()) shift the row one
      // lane down (row_shl:1, lane j <- lane j+1), then row_mirror (lane j <- lane 15 - j); lane 0's value is parked in lane 15 first
      // (row_ror:15), where the shift has no source and leaves it
      float zr[8], zi[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float pr = q > 0 ? dpp_f<0x12f>(re[(16 - q) & 15]) : re[15];
        const float pi = q > 0 ? dpp_f<0x12f>(im[(16 - q) & 15]) : im[15];
        const float tr = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(pr), __float_as_int(re[15 - q]), 0x101, 0xf, 0xf, false));
        const float ti = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(pi), __float_as_int(im[15 - q]), 0x101, 0xf, 0xf, false));
        zr[q] = dpp_f<0x140>(tr);
        zi[q] = dpp_f<0x140>(ti);
      }
      const float a = re[8], b = im[8];
      p128 = 4.0f * fmaf(b, b, a * a);
#pragma unroll
      for (int q = 0; q < 8; ++q) { re[15 - q] = zr[q]; im[15 - q] = zi[q]; }
    }
    float2 tw5[8];                                // e^{-2 pi i k/512} of my eight bins, all read before the first store to the
#pragma unroll                                    // power buffer (the compiler cannot tell the two LDS regions apart)
    for (int q = 0; q < 8; ++q) tw5[q] = s_tw512[kc + 16 * q];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float2 w = tw5[q];
      const float a = re[q], b = im[q];
      const float c = re[15 - q], d = im[15 - q];
      const float sr = a + c, si = b - d, dr = a - c, di = b + d;
      const float ur = fmaf(w.x, dr, -w.y * di);
      const float ui = fmaf(w.x, di, w.y * dr);
      const float xr = sr + ui, xi = si - ur;      // 2 X[k]
      const float yr = sr - ui, yi = si + ur;      // same modulus as 2 X[256-k]
      float pk = fmaf(xi, xi, xr * xr);            // 4 |X[k]|^2
      float pm = fmaf(yi, yi, yr * yr);            // 4 |X[256-k]|^2
      if (q == 0 && j == 0) {                      // DC / Nyquist: X[0] = a+b, X[256] = a-b
        const float v0 = 2.0f * (a + b), v1 = 2.0f * (a - b);
        pk = v0 * v0; pm = v1 * v1;
      }
      if (!USE_POWER) { pk = sqrtf(pk); pm = sqrtf(pm); }
      pb_k[(2 * kOctetFloats) * q] = pk;           // bin j + 16 q
      pb_m[-(2 * kOctetFloats) * q] = pm;          // bin 256 - j - 16 q
    }
    if (j == 0) {                                  // k = 128 pairs with itself
      s_pb[pb_pos(128)] = USE_POWER ? p128 : sqrtf(p128);
    } else if (j < 8) {
      s_pb[pb_pos(256) + j] = 0.0f;                // octet 32 is read as a whole by the mel units
    }
    wave_lds_fence();

    PH(6);                                   // untangle + power
    // next pass's PCM: issued here, where register pressure is low; the loads fly
    // during mel/DCT of this pass and the other resident waves' arithmetic
    int ntp = tp + 4;
    const bool advance = ntp >= cur_n;
    const bool more = !advance || has_next;
    if (advance) ntp = 0;
    if (more)
      pcm_prefetch<MP, ALIGNED, TYPED>(P.pcm, P.pcm_total, (advance ? nxt_samp0 : cur_samp0) + (int64_t)ntp * P.H - P.pad_left, P.H, lane, R);
    else if constexpr (TYPED) {
      // the wave's last pass (it leaves the loop below): the samples must not stay alive up to here on THIS path
      // either (see typed_loads). Not on the steady path.
#pragma unroll
      for (int m = 0; m < 2 * MP; ++m) R.v[m] = 0u;
    }

    PH(7);                                   // prefetch issue
    // ------------------------------------------------------------ mel (R6)
    {
      float a0 = 0.0f, a1 = 0.0f;                 // my two bands; a band's units are added in unit order, starting from 0
#pragma unroll
      for (int i = 0; i < UC; ++i) {
        const float4 *pp = reinterpret_cast<const float4 *>(reinterpret_cast<const unsigned char *>(s_pb) + mo[i]);
        const float4 p0 = pp[0], p1 = pp[1];
        const float4 w0 = s_melw0[i * 16 + j], w1 = s_melw1[i * 16 + j];
        float acc = p0.x * w0.x;
        acc = fmaf(p0.y, w0.y, acc); acc = fmaf(p0.z, w0.z, acc); acc = fmaf(p0.w, w0.w, acc);
        acc = fmaf(p1.x, w1.x, acc); acc = fmaf(p1.y, w1.y, acc); acc = fmaf(p1.z, w1.z, acc); acc = fmaf(p1.w, w1.w, acc);
        a0 = fmaf(acc, uf0[i], a0);
        a1 = fmaf(acc, uf1[i], a1);
      }
      PH(8);                                   // mel units
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int b = h ? band1 : band0;
        const float acc = h ? a1 : a0;
        if (b != 0xff) {
          if (PLP) {                                     // R8: floor, HTK equal loudness, power-law compression (plp.cpp:499-507)
            float v = acc * F.mel_scale;
            v = v < P.melfloor ? P.melfloor : v;
            s_lmel[b] = __expf(P.plp_compression * __logf(v * s_plp[b]));
          } else {
            s_lmel[b] = log_mel_fast(acc * F.mel_scale, P.melfloor, P.log_floor);
          }
        }
      }
      if (j + 16 >= P.n_bands) s_lmel[j + 16] = 0.0f;     // pads up to 32 for the b128 DCT reads
      if (j >= P.n_bands) s_lmel[j] = 0.0f;
    }
    wave_lds_fence();

    PH(9);                                   // band sums + log
    // ------------------------------------------------------------ PLP-CC (R8): IDFT rows (s_dct holds the cosine
    // table, same 28-float rows), then Durbin + cepstra + lifter on the group's lane 0
    if (PLP) {
      float *s_acf = s_lmel + 32;                       // 16 floats behind the padded band vector
      if (j <= P.plp_order) s_acf[j] = plp_acf_lag(s_lmel, s_dct + j * 28, P.n_bands);
      wave_lds_fence();
      if (j == 0) plp_cc_serial(s_acf, P.plp_order, s_plp + 32, s_cep);
      wave_lds_fence();
      if (j < P.n_mfcc) pend_val = s_cep[j];
    } else
    // ------------------------------------------------------------ DCT + lifter (R7)
    if (j < P.n_mfcc) {
      const float4 *row_c = reinterpret_cast<const float4 *>(s_dct + j * 28);
      const float4 *lm = reinterpret_cast<const float4 *>(s_lmel);
      float acc = 0.0f, dgain = 0.0f;
#pragma unroll
      for (int q = 0; q < 7; ++q) {
        const float4 l = lm[q], c = row_c[q];
        acc = fmaf(l.x, c.x, acc); acc = fmaf(l.y, c.y, acc); acc = fmaf(l.z, c.z, acc);
        if (q < 6) acc = fmaf(l.w, c.w, acc); else dgain = c.w;      // row[27] carries lifter * sqrt(2/nB)
      }
      pend_val = acc * dgain;
    }
    pend_live = live && j < P.n_mfcc;
    pend_row = reinterpret_cast<unsigned char *>(P.out + (cur_row0 + tp - (DELTA ? 4 : 0)) * P.ld_out);   // wave-uniform
    if constexpr (DELTA) { b_tp = tp; b_lo = cur_lo; b_live = cur_live; b_e0 = cur_e0; b_e1 = cur_e1; b_don = cur_don; }
    wave_lds_fence();   // band vector and power buffer are overwritten by the next pass's transpose
    PH(10);                                  // DCT
    if (!more) break;
    if (advance) {
      tile += tile_stride;
      cur_samp0 = nxt_samp0; cur_row0 = recs[tile].row0; cur_n = recs[tile].n_frames;
      if constexpr (DELTA) {
        cur_live = recs[tile].live_n; cur_e0 = recs[tile].e0; cur_e1 = recs[tile].e1; cur_lo = recs[tile].lo; cur_don = recs[tile].delta_on;
      }
      has_next = tile + tile_stride < n_tiles;
      if (has_next) nxt_samp0 = recs[tile + tile_stride].samp0;
    }
    tp = ntp;
  }
  if constexpr (DELTA) {                               // the last pass's rows
    float dn, ddn, drow;
    delta_exact(pend_val, d_cur, b_tp, b_lo, b_live, dn, ddn, drow);
    const int fdd = b_tp - 4 + g;
    if (j < P.n_mfcc && fdd >= b_e0 && fdd < b_e1) {
      *reinterpret_cast<float *>(pend_row + out_off) = s_prev;
      if (b_don) {
        *reinterpret_cast<float *>(pend_row + out_off_d) = drow;
        *reinterpret_cast<float *>(pend_row + out_off_dd) = ddn;
      }
    }
  } else if (pend_live) {
    uint32_t oo = out_off;
    asm volatile("" : "+v"(oo));
    *reinterpret_cast<float *>(pend_row + oo) = pend_val;
  }
  PH.flush(g_phase);
  WL.end(g_wave_life, blockIdx.x, (unsigned)wave, (unsigned)passes_done);
}

template <int MP, bool PREEMPH, bool USE_POWER, bool ALIGNED, bool PLP, int UC, bool DELTA = false>
__global__ void __launch_bounds__(kWavesPerBlock * 64, 4) lld_mfcc512(LldParams P, Fast512Tables F) {
  lld_mfcc512_body<MP, PREEMPH, USE_POWER, ALIGNED, PLP, UC, DELTA, true>(P, F);
}
template <int MP, bool PREEMPH, bool USE_POWER, bool ALIGNED, bool PLP, int UC, bool DELTA = false>
__global__ void __launch_bounds__(kWavesPerBlock * 64, 4) lld_mfcc512_padded(LldParams P, Fast512Tables F) {
  lld_mfcc512_body<MP, PREEMPH, USE_POWER, ALIGNED, PLP, UC, DELTA, false>(P, F);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
bool fast512_applicable(int Nfft, int N) { return Nfft == 512 && N <= 512 && N >= 2; }

int fast512_tile_frames() { return kTileFrames; }

// Tables of the fast kernel. Mel work units: for every band, every aligned
// octet of bins that intersects the band's bin range [rise_lo, fall_hi) is one
// unit with 8 weights (1-w on the rising run, w on the falling run, 0 outside;
// melspec.cpp:544-553). Whole bands go to lanes (at most two per lane); a lane
// adds its band's units in the order of its unit slots.
int fast512_build_host(const smilehip_lld_config &cfg, const Geometry &geo, const std::vector<float> &window,
                       const MelBank &mel, const DctTables &dct, Fast512Host &h) {
  const int pad_left = cfg.zero_pad_symmetric ? (int)((geo.Nfft - geo.N) / 2) : 0;
  const int H = (int)geo.H, N = (int)geo.N;
  if (mel.n_bands > 27 || dct.n_mfcc > 16 || cfg.win_offset != 0.0 || (pad_left & 1) || (H & 1) || H < 2) return -1;
  h.mp = (pad_left + N) <= 13 * 32 ? 13 : 16;
  const char *fp = getenv("SMILEHIP_MFCC512_FORCE_PADDED");
  h.force_padded = fp != nullptr && fp[0] == '1';
  h.tw256.resize(256);
  for (int k1 = 0; k1 < 16; ++k1)
    for (int j = 0; j < 16; ++j) {
      const double a = -2.0 * M_PI * double(j * k1) / 256.0;
      h.tw256[k1 * 16 + j] = make_float2(float(cos(a)), float(sin(a)));
    }
  h.tw512.resize(256);
  for (int k = 0; k < 256; ++k) {
    const double a = -2.0 * M_PI * double(k) / 512.0;
    h.tw512[k] = make_float2(float(cos(a)), float(sin(a)));
  }
  // window pairs with R0's 1/32767 folded in (one rounding from the double quotient)
  h.win.assign(size_t(h.mp) * 16, make_float2(0.f, 0.f));
  for (int m = 0; m < h.mp; ++m)
    for (int j = 0; j < 16; ++j) {
      const int n = 2 * (j + 16 * m) - pad_left;
      float a = 0.f, b = 0.f;
      if (n >= 0 && n < N) a = float(double(window[n]) / 32767.0);
      if (n + 1 >= 0 && n + 1 < N) b = float(double(window[n + 1]) / 32767.0);
      h.win[size_t(m) * 16 + j] = make_float2(a, b);
    }
  // mel units, band by band in octet order
  struct Unit { int octet; float w[8]; };
  std::vector<Unit> units;
  const int nb = mel.n_bands;
  std::vector<int> first_unit(nb + 1, 0);
  for (int b = 0; b < nb; ++b) {
    int lo = -1, hi = -1;
    if (mel.rise_hi[b] > mel.rise_lo[b]) { lo = mel.rise_lo[b]; hi = mel.rise_hi[b]; }
    if (mel.fall_hi[b] > mel.fall_lo[b]) { if (lo < 0) lo = mel.fall_lo[b]; hi = mel.fall_hi[b]; }
    first_unit[b] = int(units.size());
    if (lo >= 0) {
      for (int o = lo / 8; o <= (hi - 1) / 8; ++o) {
        Unit un;
        un.octet = o;
        for (int e = 0; e < 8; ++e) {
          const int n = 8 * o + e;
          float w = 0.0f;
          if (n >= mel.rise_lo[b] && n < mel.rise_hi[b]) w = 1.0f - mel.coef[n];
          else if (n >= mel.fall_lo[b] && n < mel.fall_hi[b]) w = mel.coef[n];
          un.w[e] = w;
        }
        units.push_back(un);
      }
    }
  }
  first_unit[nb] = int(units.size());
  h.n_slots = int(units.size());
  // Whole bands to lanes: at most two bands and `cap` units per lane (cap = 6 or 8: the two unit counts the kernel is
  // instantiated for). Largest band first, partnered with the largest remaining band that still fits.
  std::vector<int> size(nb), order(nb);
  for (int b = 0; b < nb; ++b) { size[b] = first_unit[b + 1] - first_unit[b]; order[b] = b; }
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return size[x] > size[y]; });
  int cap = 0;
  std::vector<std::pair<int, int>> lanes;          // (first band, second band or -1)
  for (int c : {6, 8}) {
    lanes.clear();
    std::vector<char> used(nb, 0);
    bool ok = true;
    for (int oi = 0; oi < nb && ok; ++oi) {
      const int a = order[oi];
      if (used[a]) continue;
      used[a] = 1;
      if (size[a] > c) { ok = false; break; }
      int partner = -1;
      for (int oj = oi + 1; oj < nb; ++oj)
        if (!used[order[oj]] && size[a] + size[order[oj]] <= c) { partner = order[oj]; break; }
      if (partner >= 0) used[partner] = 1;
      lanes.push_back({a, partner});
    }
    if (ok && (int)lanes.size() <= 16) { cap = c; break; }
  }
  if (cap == 0) return -1;
  h.mel_units = cap;
  // Unit slots. At step i the 16 lanes of a frame issue one ds_read_b128 each (and a second one 16 bytes further on);
  // the hardware serves the 16 lanes of a b128 lane group in one cycle iff they touch 16 different bank quads, and octet o
  // sits on quad 3 o mod 16 of its frame's buffer (all four buffers of a wave start on the same bank): a step is
  // conflict-free iff its 16 octets differ mod 16. The order of a lane's units is free (it only fixes the order of a
  // band's additions), so: start from octet order, then swap slot pairs of one lane while that lowers
  // (worst multiplicity per step, number of colliding lanes), lexicographically -- deterministic hill climbing.
  std::vector<std::vector<int>> slot(16, std::vector<int>(cap, -1));       // unit index or -1 (padding)
  for (size_t l = 0; l < lanes.size(); ++l) {
    int pos = 0;
    for (int which = 0; which < 2; ++which) {
      const int b = which ? lanes[l].second : lanes[l].first;
      if (b < 0) continue;
      for (int c = first_unit[b]; c < first_unit[b + 1]; ++c) slot[l][pos++] = c;
    }
  }
  auto step_cost = [&](int i, int &worst, int &coll) {
    int cnt[16] = {0};
    for (int l = 0; l < 16; ++l)
      if (slot[l][i] >= 0) ++cnt[units[slot[l][i]].octet & 15];
    worst = 1; coll = 0;
    for (int r = 0; r < 16; ++r) { worst = std::max(worst, cnt[r]); coll += std::max(0, cnt[r] - 1); }
  };
  auto total_cost = [&](long &primary, long &secondary) {
    primary = secondary = 0;
    for (int i = 0; i < cap; ++i) { int w, c; step_cost(i, w, c); primary += w; secondary += c; }
  };
  long best_p, best_s;
  total_cost(best_p, best_s);
  for (bool improved = true; improved;) {
    improved = false;
    for (int l = 0; l < 16; ++l)
      for (int a = 0; a < cap; ++a)
        for (int b = a + 1; b < cap; ++b) {
          if (slot[l][a] == slot[l][b]) continue;
          std::swap(slot[l][a], slot[l][b]);
          long p, s2;
          total_cost(p, s2);
          if (p < best_p || (p == best_p && s2 < best_s)) { best_p = p; best_s = s2; improved = true; }
          else std::swap(slot[l][a], slot[l][b]);
        }
  }
  h.mel_conflict_steps = int(best_p - cap);         // extra LDS cycles per b128 read group and pass, 0 = conflict-free
  if (getenv("SMILEHIP_DEBUG_TABLES"))
    fprintf(stderr, "fast512: %d mel units on %zu lanes, %d per lane, bank model: %ld extra cycles over %d steps (%ld colliding lanes)\n",
            h.n_slots, lanes.size(), cap, best_p - cap, cap, best_s);
  h.melw.assign(size_t(cap) * 16 * 2, make_float4(0.f, 0.f, 0.f, 0.f));
  h.melo.assign(size_t(cap) * 16, 0u);
  h.lane_bands.assign(16, int32_t(0xffff00));        // no units, no bands
  for (int i = 0; i < cap; ++i) {
    bool taken[16] = {false};
    for (int l = 0; l < 16; ++l)
      if (slot[l][i] >= 0) taken[units[slot[l][i]].octet & 15] = true;
    for (int l = 0; l < 16; ++l) {
      const size_t idx = size_t(i) * 16 + l;
      if (slot[l][i] >= 0) {
        const Unit &un = units[slot[l][i]];
        h.melw[2 * idx] = make_float4(un.w[0], un.w[1], un.w[2], un.w[3]);
        h.melw[2 * idx + 1] = make_float4(un.w[4], un.w[5], un.w[6], un.w[7]);
        h.melo[idx] = uint32_t(un.octet) * uint32_t(kOctetFloats * 4);
      } else {                                       // padding unit: zero weights on an octet whose bank quad is still free
        int o = 0;
        for (int r = 0; r < 16; ++r)
          if (!taken[r]) { o = r; taken[r] = true; break; }
        h.melo[idx] = uint32_t(o) * uint32_t(kOctetFloats * 4);
      }
    }
  }
  if (getenv("SMILEHIP_DEBUG_TABLES")) {             // the table tools/lds_bank_sim.py prices the power-buffer reads with
    fprintf(stderr, "fast512: unit octets [step][lane]:");
    for (size_t idx = 0; idx < h.melo.size(); ++idx) fprintf(stderr, " %u", h.melo[idx] / uint32_t(kOctetFloats * 4));
    fprintf(stderr, "\n");
  }
  for (size_t l = 0; l < lanes.size(); ++l) {
    uint32_t mask = 0;
    const int b0 = lanes[l].first;
    for (int i = 0; i < cap; ++i)
      if (slot[l][i] >= first_unit[b0] && slot[l][i] < first_unit[b0 + 1]) mask |= 1u << i;
    h.lane_bands[l] = int32_t(mask | (uint32_t(b0) << 8) | (uint32_t(lanes[l].second < 0 ? 0xff : lanes[l].second) << 16));
  }
  // the kernel leaves 4|X|^2 (or 2|X| without usePower) in the power buffer
  h.mel_scale = mel.scale * (cfg.use_power ? 0.25f : 0.5f);
  h.dct28.assign(16 * 28, 0.0f);
  for (int r = 0; r < dct.n_mfcc; ++r)
    for (int m = 0; m < mel.n_bands; ++m) h.dct28[size_t(r) * 28 + m] = dct.cos_rows[size_t(r) * mel.n_bands + m];
  for (int r = 0; r < dct.n_mfcc; ++r) h.dct28[size_t(r) * 28 + 27] = dct.gain[r];     // read with the row's last b128
  return 0;
}

template <int MP, bool PREEMPH, bool USE_POWER, bool ALIGNED, bool PLP, int UC, bool DELTA = false>
static hipError_t launch_mfcc512_one(bool padded, unsigned grid, hipStream_t s, const LldParams &P, const Fast512Tables &F) {
  constexpr int shared_floats = 256 * 2 + MP * 16 * 2 + 256 * 2 + UC * 16 * 8 + 16 * 28 + 48;          // (the kernel's own figure)
  constexpr int wave_floats = split_transpose<MP, PLP, DELTA>() ? kTSWaveFloats : kWaveFloats;
  constexpr size_t lds = sizeof(float) * (size_t(shared_floats) + size_t(kWavesPerBlock) * wave_floats);
  static_assert(2 * lds <= 160 * 1024, "two blocks per CU");
  if constexpr (PREEMPH) {
    if (padded) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_mfcc512_padded<MP, PREEMPH, USE_POWER, ALIGNED, PLP, UC, DELTA>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      SMILEHIP_KLAUNCH((lld_mfcc512_padded<MP, PREEMPH, USE_POWER, ALIGNED, PLP, UC, DELTA>), dim3(grid), dim3(kWavesPerBlock * 64), lds, s, P, F);
      return hipSuccess;
    }
  }
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_mfcc512<MP, PREEMPH, USE_POWER, ALIGNED, PLP, UC, DELTA>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  SMILEHIP_KLAUNCH((lld_mfcc512<MP, PREEMPH, USE_POWER, ALIGNED, PLP, UC, DELTA>), dim3(grid), dim3(kWavesPerBlock * 64), lds, s, P, F);
  return hipSuccess;
}

hipError_t launch_mfcc512(const LldParams &P, const Fast512Tables &F, const Fast512Host &h, bool aligned, bool fused_delta, hipStream_t s) {
  if (fused_delta && (!aligned || !P.ftile_rec || P.n_ftiles <= 0)) return hipErrorInvalidValue;   // (the caller decides; see smilehip_mfcc_run)
  unsigned grid = (unsigned)(((fused_delta ? P.n_ftiles : P.n_tiles) + kWavesPerBlock - 1) / kWavesPerBlock);
  if (grid > (unsigned)h.max_blocks) grid = (unsigned)h.max_blocks;   // persistent: 2 blocks of 8 waves per CU
#ifdef SMILEHIP_DEBUG_KNOBS
  if (const char *e = getenv("SMILEHIP_DEBUG_GRID")) grid = (unsigned)atoi(e);
#endif
  bool launched = false;
  // pad_left = 0 (frame sample 0 in lane 0, register 0): lld_mfcc512; symmetric zero padding: lld_mfcc512_padded (PREEMPH only:
  // without pre-emphasis there is no fix-up and the two kernels are the same code)
  const bool padded = P.pad_left != 0 || h.force_padded;
#define SMILEHIP_LAUNCH(...)                                                                                    \
  {                                                                                                             \
    hipError_t e = launch_mfcc512_one<__VA_ARGS__>(padded, grid, s, P, F);                                      \
    if (e != hipSuccess) return e;                                                                              \
    launched = true;                                                                                            \
  }
#define SMILEHIP_MATCH(MPV, PE, UP, AL, PL, UCV)                                                                \
  (!launched && h.mp == MPV && (P.preemph != 0) == PE && (P.use_power != 0) == UP && aligned == AL && (P.plp != 0) == PL && h.mel_units == UCV)
  // the delta-fused instances exist for dword-aligned input (every shipped geometry of the bench and the file front end)
#define SMILEHIP_PICK_UD(MPV, PE, UP, PL, UCV) \
  if (fused_delta && SMILEHIP_MATCH(MPV, PE, UP, true, PL, UCV)) SMILEHIP_LAUNCH(MPV, PE, UP, true, PL, UCV, true)
#define SMILEHIP_PICK_U(MPV, PE, UP, AL, PL, UCV) \
  if (!fused_delta && SMILEHIP_MATCH(MPV, PE, UP, AL, PL, UCV)) SMILEHIP_LAUNCH(MPV, PE, UP, AL, PL, UCV)
#define SMILEHIP_PICK(MPV, PE, UP, AL, PL) SMILEHIP_PICK_U(MPV, PE, UP, AL, PL, 6) SMILEHIP_PICK_U(MPV, PE, UP, AL, PL, 8)
#define SMILEHIP_PICKD(MPV, PE, UP, PL) SMILEHIP_PICK_UD(MPV, PE, UP, PL, 6) SMILEHIP_PICK_UD(MPV, PE, UP, PL, 8)
#define SMILEHIP_PICK2(MPV, PE, UP) SMILEHIP_PICK(MPV, PE, UP, true, false) SMILEHIP_PICK(MPV, PE, UP, false, false) SMILEHIP_PICKD(MPV, PE, UP, false)
#define SMILEHIP_PICK4(MPV) SMILEHIP_PICK2(MPV, true, true) SMILEHIP_PICK2(MPV, true, false) \
                            SMILEHIP_PICK2(MPV, false, true) SMILEHIP_PICK2(MPV, false, false) \
                            /* the PLP chain works on the power spectrum (the plan checks use_power) */ \
                            SMILEHIP_PICK(MPV, true, true, true, true) SMILEHIP_PICK(MPV, true, true, false, true) \
                            SMILEHIP_PICK(MPV, false, true, true, true) SMILEHIP_PICK(MPV, false, true, false, true) \
                            SMILEHIP_PICKD(MPV, true, true, true) SMILEHIP_PICKD(MPV, false, true, true)
  SMILEHIP_PICK4(13)
  SMILEHIP_PICK4(16)
#undef SMILEHIP_PICK4
#undef SMILEHIP_PICK2
#undef SMILEHIP_PICKD
#undef SMILEHIP_PICK
#undef SMILEHIP_PICK_U
#undef SMILEHIP_PICK_UD
#undef SMILEHIP_MATCH
#undef SMILEHIP_LAUNCH
  if (!launched) return hipErrorInvalidConfiguration;     // no instantiation for this geometry: fail, never skip
  return hipGetLastError();
}

}  // namespace smilehip
