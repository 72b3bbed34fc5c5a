// Eval video (include/lhw.h: lhw_jpeg_encode): the entropy-coded segments of baseline JPEG frames, coded where the ray caster left the
// pixels.  The arithmetic -- colour conversion, 4:2:0 sampling, the integer DCT, quantisation, Huffman coding, restart markers, byte
// stuffing -- is specified in include/lhw.h; this file adds only how the work is laid out.
//
// Lane mapping: one wavefront per (frame, MCU row).  A restart marker closes every MCU row, so the rows are independent bit streams.
// The row's 6 M blocks are taken in passes of 64, a lane per block, in stream order (block b = 6 mcu + slot).  In a pass a lane
//   1. fetches its block's samples (a Y lane 64 pixels, a chroma lane 256) into its own column of an LDS tile [64 coefficients][64 lanes],
//      runs the row and the column pass of the DCT on that column with eight values in registers at a time, and quantises in place;
//   2. leaves its DC value in LDS, from where the next block of the same component (1, 3 or 6 blocks on; the last eight values are
//      carried into the next pass) takes its prediction;
//   3. walks its coefficients in zig-zag order once to count the bits of its code; a wave-wide prefix sum (ds_bpermute) turns the counts
//      into bit offsets;
//   4. walks them again and ORs the code words, big-endian, into the pass's bit buffer in LDS (64 x 208 bytes: the bound of lhw.h).
// The wave then reads the buffer's complete bytes 64 at a time, a ballot marks the FF bytes, a popcount of the lower lanes gives every
// byte its stuffed position, and the bytes go to the row's slot in scratch; up to seven left-over bits open the next pass's buffer.
// The last pass pads with 1-bits and appends RSTm.  jpeg_scan_kernel (one wavefront) turns the row sizes into offsets, jpeg_pack_kernel copies the
// rows to their places.  No state, no host synchronisation.
#include "lhw_internal.h"

namespace {

enum { BLOCK_BITS = 1660, PASS_WORDS = (7 + 64 * BLOCK_BITS + 31) / 32 + 1 };
static_assert(2 * ((6 * BLOCK_BITS + 7) / 8) + 2 <= LHW_JPEG_MCU_BYTES + 4, "lhw.h's bound on an MCU row of one MCU");

// ITU-T T.81 Annex K: BITS (codes per length 1..16) and HUFFVAL of tables K.3 / K.4 (DC) and K.5 / K.6 (AC), luminance then chrominance
constexpr uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// What the kernel looks up: per table and symbol (code length << 16) | code, the canonical codes of Annex C; and the zig-zag order
struct Tables {
  uint32_t dc[2][16];
  uint32_t ac[2][256];
  uint8_t zigzag[64];      // natural index of the k-th coefficient in zig-zag order
};
constexpr Tables make_tables() {
  Tables t{};
  for (int c = 0; c < 2; c++) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++, code <<= 1)
      for (int i = 0; i < DC_BITS[c][len - 1]; i++) t.dc[c][k++] = ((uint32_t)len << 16) | code++;      // (HUFFVAL of a DC table is 0..11)
    code = 0;
    k = 0;
    for (int len = 1; len <= 16; len++, code <<= 1)
      for (int i = 0; i < AC_BITS[c][len - 1]; i++) t.ac[c][AC_VALS[c][k++]] = ((uint32_t)len << 16) | code++;
  }
  int x = 0, y = 0;
  for (int k = 0; k < 64; k++) {
    t.zigzag[k] = (uint8_t)(8 * y + x);
    if ((x + y) % 2 == 0) {      // moving up and to the right
      if (x == 7) y++; else if (y == 0) x++; else { x++; y--; }
    } else {
      if (y == 7) x++; else if (x == 0) y++; else { x--; y++; }
    }
  }
  return t;
}
__device__ const Tables kTables = make_tables();

struct JpegArgs {
  int W, H, M, R;
  long long row_stride;
  const uint8_t* rgb;
  uint8_t* rows;
  int32_t* sizes;
  uint32_t q8[64];      // 8 q per natural index: luminance in the low half, chrominance in the high half
};

__device__ __forceinline__ int D(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One 1-D pass of include/lhw.h's DCT on eight values in registers
template <int PASS>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
  constexpr int n = PASS == 1 ? 11 : 15;
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int e0 = t0 + t3, e3 = t0 - t3, e1 = t1 + t2, e2 = t1 - t2, z = (e2 + e3) * 4433;
  d[0] = PASS == 1 ? (e0 + e1) * 4 : D(e0 + e1, 2);
  d[4] = PASS == 1 ? (e0 - e1) * 4 : D(e0 - e1, 2);
  d[2] = D(z + e3 * 6270, n);
  d[6] = D(z - e2 * 15137, n);
  const int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) * 9633;
  const int a3 = z5 - z3 * 16069, a4 = z5 - z4 * 3196;
  d[7] = D(t4 * 2446 - z1 * 7373 + a3, n);
  d[5] = D(t5 * 16819 - z2 * 20995 + a4, n);
  d[3] = D(t6 * 25172 - z2 * 20995 + a3, n);
  d[1] = D(t7 * 12299 - z1 * 7373 + a4, n);
}

// component c (0 Y, 1 Cb, 2 Cr) of the pixel at p
__device__ __forceinline__ int ycc(const uint8_t* p, int c) {
  const int r = p[0], g = p[1], b = p[2];
  if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16;
}

// The bits of one block's code, most significant first, on their way into the pass's bit buffer: `fill` pending bits in the top of `acc`,
// bound for word `w`.  Neighbouring blocks share a word, hence the OR.
struct BitSink {
  int* buf;
  int w, fill;
  unsigned long long acc;
  __device__ __forceinline__ void put(unsigned v, int n) {
    acc |= (unsigned long long)v << (64 - fill - n);
    fill += n;
    if (fill >= 32) {
      atomicOr(&buf[w++], (int)(unsigned)(acc >> 32));
      acc <<= 32;
      fill -= 32;
    }
  }
  __device__ __forceinline__ void flush() {
    if (fill > 0) atomicOr(&buf[w], (int)(unsigned)(acc >> 32));
  }
};

__device__ __forceinline__ int bit_length(int v) { return 32 - __clz(v); }      // of v >= 0

// The code of the lane's block: returns its length in bits and, if EMIT, puts the bits into `sink`
template <bool EMIT>
__device__ __forceinline__ int code_block(const short* coef, int lane, int diff, const unsigned* dc, const unsigned* ac, const unsigned char* zigzag,
                                          BitSink& sink) {
  int bits = 0;
  auto put = [&](unsigned entry, int value, int s) {      // a table entry, then the s low bits of value (value - 1 if negative)
    const int len = (int)(entry >> 16) + s;
    bits += len;
    if (EMIT) sink.put(((entry & 0xffffu) << s) | ((unsigned)(value < 0 ? value - 1 : value) & ((1u << s) - 1u)), len);
  };
  const int sd = bit_length(diff < 0 ? -diff : diff);
  put(dc[sd], diff, sd);
  int run = 0;
  for (int k = 1; k < 64; k++) {
    const int c = coef[zigzag[k] * 64 + lane];
    if (c == 0) {
      run++;
      continue;
    }
    for (; run >= 16; run -= 16) put(ac[0xF0], 0, 0);
    const int s = bit_length(c < 0 ? -c : c);
    put(ac[(run << 4) | s], c, s);
    run = 0;
  }
  if (run > 0) put(ac[0x00], 0, 0);
  return bits;
}

__device__ __forceinline__ int lane_value(int v, int src_lane) { return __builtin_amdgcn_ds_bpermute(src_lane << 2, v); }

// inclusive prefix sum over the wave's 64 lanes
__device__ __forceinline__ int wave_scan(int v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const int t = lane_value(v, lane >= d ? lane - d : lane);
    if (lane >= d) v += t;
  }
  return v;
}

__global__ void __launch_bounds__(64) jpeg_rows_kernel(JpegArgs a) {
  __shared__ short s_coef[64 * 64];      // [coefficient, natural order][lane]
  __shared__ int s_bits[PASS_WORDS];     // the pass's bit stream: stream bit i is bit 31 - i % 32 of word i / 32
  __shared__ unsigned s_dc[2][16], s_ac[2][256];
  __shared__ unsigned s_q8[64];
  __shared__ unsigned char s_zigzag[64];
  __shared__ int s_pred[72];             // DC values: [8 + lane] of this pass, [0..8) the last eight of the pass before
  LHW_LDS_POISON(s_coef);
  LHW_LDS_POISON(s_bits);
  LHW_LDS_POISON(s_dc);
  LHW_LDS_POISON(s_ac);
  LHW_LDS_POISON(s_q8);
  LHW_LDS_POISON(s_zigzag);
  LHW_LDS_POISON(s_pred);
  const int lane = (int)threadIdx.x;
  const int f = (int)(blockIdx.x / (unsigned)a.R), row = (int)(blockIdx.x % (unsigned)a.R);
  for (int i = lane; i < 512; i += 64) (&s_ac[0][0])[i] = (&kTables.ac[0][0])[i];
  if (lane < 32) (&s_dc[0][0])[lane] = (&kTables.dc[0][0])[lane];
  s_zigzag[lane] = kTables.zigzag[lane];
#pragma unroll
  for (int i = 0; i < 64; i++) s_q8[i] = a.q8[i];      // (kernel arguments: the same value from every lane)
  if (lane < 8) s_pred[lane] = 0;
  __syncthreads();

  const int W = a.W, H = a.H;
  const uint8_t* img = a.rgb + (size_t)f * (size_t)H * (size_t)W * 3;
  uint8_t* out = a.rows + (size_t)blockIdx.x * (size_t)a.row_stride;
  const int nblocks = 6 * a.M, passes = (nblocks + 63) / 64;
  int written = 0;                       // bytes of this row in `out` so far
  int carry_bits = 0;                    // bits (< 8) the pass before left over; they are the top bits of carry_byte
  unsigned carry_byte = 0;

  for (int p = 0; p < passes; p++) {
    const int b = p * 64 + lane, mcu = b / 6, slot = b % 6;
    const bool active = b < nblocks;
    const int table = slot < 4 ? 0 : 1;
    short* col = s_coef + lane;
    if (active) {
      if (slot < 4) {
        const int x0 = mcu * 16 + (slot & 1) * 8, y0 = row * 16 + (slot >> 1) * 8;
        for (int j = 0; j < 8; j++) {
          const uint8_t* line = img + (size_t)min(y0 + j, H - 1) * (size_t)W * 3;
          for (int i = 0; i < 8; i++) col[(8 * j + i) * 64] = (short)(ycc(line + (size_t)min(x0 + i, W - 1) * 3, 0) - 128);
        }
      } else {
        const int x0 = mcu * 16, y0 = row * 16, c = slot - 3;
        for (int j = 0; j < 8; j++) {
          const uint8_t* line0 = img + (size_t)min(y0 + 2 * j, H - 1) * (size_t)W * 3;
          const uint8_t* line1 = img + (size_t)min(y0 + 2 * j + 1, H - 1) * (size_t)W * 3;
          for (int i = 0; i < 8; i++) {
            const size_t xa = (size_t)min(x0 + 2 * i, W - 1) * 3, xb = (size_t)min(x0 + 2 * i + 1, W - 1) * 3;
            col[(8 * j + i) * 64] = (short)(((ycc(line0 + xa, c) + ycc(line0 + xb, c) + ycc(line1 + xa, c) + ycc(line1 + xb, c) + 2) >> 2) - 128);
          }
        }
      }
      for (int j = 0; j < 8; j++) {      // pass 1: rows
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; i++) d[i] = col[(8 * j + i) * 64];
        fdct8<1>(d);
#pragma unroll
        for (int i = 0; i < 8; i++) col[(8 * j + i) * 64] = (short)d[i];
      }
      for (int i = 0; i < 8; i++) {      // pass 2: columns, then the quantiser
        int d[8];
#pragma unroll
        for (int j = 0; j < 8; j++) d[j] = col[(8 * j + i) * 64];
        fdct8<2>(d);
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const int q8 = (int)((s_q8[8 * j + i] >> (16 * table)) & 0xffffu);
          const int k = ((d[j] < 0 ? -d[j] : d[j]) + (q8 >> 1)) / q8;
          col[(8 * j + i) * 64] = (short)(d[j] < 0 ? -k : k);
        }
      }
    }
    const int dcv = active ? col[0] : 0;
    s_pred[8 + lane] = dcv;
    __syncthreads();
    // the previous block of the same component: Y follows Y (across the MCU boundary: 3 back), Cb and Cr their own in the MCU before
    const int back = slot == 0 ? 3 : (slot < 4 ? 1 : 6);
    const int diff = dcv - (((slot >= 1 && slot <= 3) || mcu > 0) ? s_pred[8 + lane - back] : 0);
    BitSink sink{s_bits, 0, 0, 0ull};
    const int len = active ? code_block<false>(s_coef, lane, diff, s_dc[table], s_ac[table], s_zigzag, sink) : 0;
    const int end = wave_scan(len, lane);
    const int avail = carry_bits + lane_value(end, 63);      // the bits of this pass's buffer
    __syncthreads();                                         // (every prediction is read)
    if (lane < 8) s_pred[lane] = s_pred[64 + lane];
    for (int w = lane; w < (avail + 31) / 32 + 1; w += 64) s_bits[w] = w == 0 ? (int)(carry_byte << 24) : 0;
    __syncthreads();
    if (active) {
      const int pos = carry_bits + end - len;
      sink.w = pos >> 5;
      sink.fill = pos & 31;
      code_block<true>(s_coef, lane, diff, s_dc[table], s_ac[table], s_zigzag, sink);
      sink.flush();
    }
    const bool last = p == passes - 1;
    int nbytes = avail >> 3, left = avail & 7;
    if (last && left) {      // the end of the restart interval: 1-bits up to the byte boundary
      if (lane == 0) atomicOr(&s_bits[nbytes >> 2], (int)((0xffu >> left) << (24 - 8 * (nbytes & 3))));
      nbytes++;
      left = 0;
    }
    __syncthreads();
    for (int t = 0; t < nbytes; t += 64) {      // complete bytes leave, every FF followed by 00
      const int i = t + lane;
      const bool in = i < nbytes;
      const unsigned byte = in ? ((unsigned)s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu : 0u;
      const unsigned long long ff = __ballot(in && byte == 0xffu);
      const int o = written + lane + __popcll(ff & ((1ull << lane) - 1ull));
      if (in) {
        out[o] = (uint8_t)byte;
        if (byte == 0xffu) out[o + 1] = 0;
      }
      written += min(64, nbytes - t) + __popcll(ff);
    }
    carry_bits = left;
    carry_byte = left ? ((unsigned)s_bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 0xffu : 0u;
  }
  if (lane == 0) {
    if (row != a.R - 1) {
      out[written] = 0xff;
      out[written + 1] = (uint8_t)(0xd0 + (row & 7));
      written += 2;
    }
    a.sizes[blockIdx.x] = written;
  }
}

// offsets [n + 1] = the exclusive prefix sum of sizes [n]; frame_offset [F + 1] = every R-th of them.  One wavefront, 64 rows a step.
__global__ void __launch_bounds__(64) jpeg_scan_kernel(const int32_t* sizes, long long* offsets, long long* frame_offset, int n, int R) {
  const int lane = (int)threadIdx.x;
  long long base = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const int v = i < n ? sizes[i] : 0;
    const int end = wave_scan(v, lane);
    if (i < n) {
      offsets[i] = base + (end - v);
      if (i % R == 0) frame_offset[i / R] = base + (end - v);
    }
    base += lane_value(end, 63);
  }
  if (lane == 0) {
    offsets[n] = base;
    frame_offset[n / R] = base;
  }
}

__global__ void __launch_bounds__(64) jpeg_pack_kernel(const uint8_t* rows, long long row_stride, const int32_t* sizes, const long long* offsets, uint8_t* out) {
  const uint8_t* src = rows + (size_t)blockIdx.x * (size_t)row_stride;
  uint8_t* dst = out + offsets[blockIdx.x];
  const int n = sizes[blockIdx.x];
  for (int i = (int)threadIdx.x; i < n; i += 64) dst[i] = src[i];
}

// 0 if the settings are valid, else the message is set
int check_settings(const LhwJpegSettings* s, int32_t F, const char* who) {
  if (!s) return lhw_fail(LHW_ERR_ARG, "%s: settings is NULL", who);
  if (F < 0) return lhw_fail(LHW_ERR_ARG, "%s: F = %d", who, F);
  if (s->width < 1 || s->height < 1 || s->width > 65535 || s->height > 65535)
    return lhw_fail(LHW_ERR_ARG, "%s: image size %d x %d (a JPEG frame is 1..65535 each way)", who, s->width, s->height);
  for (int t = 0; t < 2; t++)
    for (int i = 0; i < 64; i++)
      if (s->qtable[t][i] < 1 || s->qtable[t][i] > 255)
        return lhw_fail(LHW_ERR_ARG, "%s: qtable[%d][%d] = %d (baseline tables hold 1..255)", who, t, i, (int)s->qtable[t][i]);
  const long long rows = (long long)F * ((s->height + 15) / 16);
  if (rows > 0x7fffffffLL) return lhw_fail(LHW_ERR_ARG, "%s: %d frames of %d MCU rows exceed one launch", who, F, (s->height + 15) / 16);
  return LHW_OK;
}

long long row_stride(const LhwJpegSettings* s) { return (long long)LHW_JPEG_MCU_BYTES * ((s->width + 15) / 16) + 4; }
long long total_rows(const LhwJpegSettings* s, int32_t F) { return (long long)F * ((s->height + 15) / 16); }

}  // namespace

extern "C" int64_t lhw_jpeg_out_bytes(const LhwJpegSettings* s, int32_t F) {
  if (check_settings(s, F, "lhw_jpeg_out_bytes") != LHW_OK) return -1;
  return total_rows(s, F) * row_stride(s);
}

extern "C" int64_t lhw_jpeg_scratch_bytes(const LhwJpegSettings* s, int32_t F) {
  if (check_settings(s, F, "lhw_jpeg_scratch_bytes") != LHW_OK) return -1;
  return F == 0 ? 0 : total_rows(s, F) * row_stride(s) + 16 * (total_rows(s, F) + 1);
}

extern "C" int lhw_jpeg_encode(const LhwJpegSettings* s, int32_t F, const uint8_t* rgb_dev, uint8_t* scratch_dev, int64_t scratch_bytes,
                               uint8_t* out_dev, int64_t out_capacity, int64_t* frame_offset_dev, void* stream) {
  if (int rc = check_settings(s, F, "lhw_jpeg_encode")) return rc;
  if (F == 0) return LHW_OK;
  if (!rgb_dev || !scratch_dev || !out_dev || !frame_offset_dev) return lhw_fail(LHW_ERR_ARG, "lhw_jpeg_encode: a required buffer is NULL");
  if (((uintptr_t)scratch_dev & 7) != 0) return lhw_fail(LHW_ERR_ARG, "lhw_jpeg_encode: scratch_dev is not 8-byte aligned");
  const long long n = total_rows(s, F), need_out = n * row_stride(s), need_scratch = need_out + 16 * (n + 1);
  if (scratch_bytes < need_scratch)
    return lhw_fail(LHW_ERR_ARG, "lhw_jpeg_encode: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, need_scratch);
  if (out_capacity < need_out)
    return lhw_fail(LHW_ERR_ARG, "lhw_jpeg_encode: output capacity of %lld bytes, %lld needed", (long long)out_capacity, need_out);
  hipStream_t st = (hipStream_t)stream;
  JpegArgs a;
  a.W = s->width; a.H = s->height; a.M = (a.W + 15) / 16; a.R = (a.H + 15) / 16;
  a.row_stride = row_stride(s);
  a.rgb = rgb_dev;
  long long* offsets = (long long*)scratch_dev;
  a.sizes = (int32_t*)(scratch_dev + 8 * (n + 1));
  a.rows = scratch_dev + 16 * (n + 1);
  for (int i = 0; i < 64; i++) a.q8[i] = 8u * s->qtable[0][i] | (8u * s->qtable[1][i]) << 16;
  hipLaunchKernelGGL(jpeg_rows_kernel, dim3((unsigned)n), dim3(64), 0, st, a);
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(64), 0, st, (const int32_t*)a.sizes, offsets, (long long*)frame_offset_dev, (int)n, a.R);
  hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)n), dim3(64), 0, st, (const uint8_t*)a.rows, a.row_stride, (const int32_t*)a.sizes,
                     (const long long*)offsets, out_dev);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}
