// Baseline JPEG encoder for the sample writers: uint8 RGB [N, H, W, 3] -> the entropy-coded data + EOI of the file PIL.Image.save(path) writes for each image
// (quality 75 unless asked, 4:2:0, Annex-K tables, no restart markers), byte for byte; the 623 header bytes are the host's (io_formats.jpeg_header).  libjpeg's
// default path is integer arithmetic end to end, so "the same bytes" is a matter of doing the same integer operations, and DESIGN.md ("JPEG encode") lists them.
//
// Six launches, all on the caller's stream, no host synchronisation, no set-up (static LDS only; the tables are constant-initialised device globals):
//   1 jpeg_coef_kernel    colour, 2x2 down-sampling, jfdctint, quantisation -> int16 coefficients, zig-zag inside a block, blocks in scan order (per MCU: four Y,
//                         Cb, Cr; dummy blocks included), so that everything after it walks one flat array.
//                         A wave owns one MCU, a workgroup four adjacent ones: its 16 x 64-pixel strip is read once, 16 bytes per lane when the rows are
//                         16-byte aligned (W % 16 == 0), into the LDS; a lane converts one 2x2 quad (four Y, one Cb, one Cr); lanes 0..47 then run the row pass of
//                         one (block, row) each and, after the transposition through the LDS (row stride 9 words: the column reads hit distinct banks), the column
//                         pass and quantisation of one (block, column); the MCU's 768 bytes leave as 48 16-byte stores.
//   2 jpeg_bits_kernel    one thread per block: the number of bits its Huffman codes take.
//   3 jpeg_scan_bits      one workgroup per image walks its blocks in tiles of 256: exclusive scan in place -> every block's bit offset, and the total.
//   4 jpeg_pack_kernel    a workgroup per 2 KiB chunk of the (unstuffed) stream: finds the blocks that overlap the chunk (binary search in the offsets), every
//                         thread codes one block at a time and ORs its codes into the chunk's words in the LDS at the block's own bit offset (atomicOr on LDS words:
//                         order-independent, so deterministic); pads the last byte with 1-bits; stores the chunk (only chunks that can reach `cap`: a stuffed byte
//                         never lies before its unstuffed place) and counts its 0xFF bytes.
//   5 jpeg_scan_ff        per image: exclusive scan of the chunks' 0xFF counts; lengths[i] = bytes + 0xFF bytes + 2, whatever `cap` is.
//   6 jpeg_stuff_kernel   per stored chunk: every thread copies 8 bytes to their stuffed place (chunk base + 0xFF bytes before it), a 0x00 behind every 0xFF, FF D9
//                         behind the last byte; nothing at or beyond `cap`.
// Bit offsets fit 32 bits: at most 6 * 65536 blocks (4096 x 4096) of at most 1660 bits (63 x (16 + 10) + 11 + 11) < 2^30.  Element offsets into the
// workspace and `out` are computed in size_t.
#pragma once
#include "common.h"

#define JPEG_CHUNK 2048                  // bytes of unstuffed stream per workgroup of the pack / stuff kernels: 256 threads x 8 bytes
#define JPEG_CHUNK_WORDS (JPEG_CHUNK / 4)
#define JPEG_BLOCK_MAX_BYTES 216         // > 1660 bits: bounds the chunks an image can have
#define JPEG_MAX_DIM 4096

// ITU-T T.81 Annex K: K.1 / K.2 (natural order), the zig-zag scan, K.3-K.6 as "sixteen code counts, then the symbols" -- the same strings as io_formats.JPEG_HUFFMAN
// (tests/test_jpeg_ref.py compares them)
static __device__ const unsigned char g_jpeg_qbase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
struct JpegZigzag {
  unsigned char pos[64];  // natural index -> place in the zig-zag scan
};
constexpr JpegZigzag jpeg_make_zigzag() {
  constexpr unsigned char zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  JpegZigzag z{};
  for (int k = 0; k < 64; ++k) z.pos[zz[k]] = (unsigned char)k;
  return z;
}
static __device__ const JpegZigzag g_jpeg_zigzag = jpeg_make_zigzag();

struct JpegHuffTab {
  unsigned int e[256];  // symbol -> code | length << 16 (T.81 Annex C); 0 = no such symbol
};
constexpr int jpeg_hex(char c) { return c >= 'a' ? c - 'a' + 10 : c - '0'; }
constexpr JpegHuffTab jpeg_make_huff(const char* spec) {
  JpegHuffTab t{};
  unsigned code = 0;
  int k = 16;  // byte index of the next symbol
  for (int len = 1; len <= 16; ++len) {
    const int count = jpeg_hex(spec[2 * (len - 1)]) * 16 + jpeg_hex(spec[2 * (len - 1) + 1]);
    for (int i = 0; i < count; ++i, ++k, ++code) t.e[jpeg_hex(spec[2 * k]) * 16 + jpeg_hex(spec[2 * k + 1])] = code | (unsigned)len << 16;
    code <<= 1;
  }
  return t;
}
#define JPEG_DHT_DC_LUMA "00010501010101010100000000000000" "000102030405060708090a0b"
#define JPEG_DHT_AC_LUMA                                                                                                                   \
  "0002010303020403050504040000017d"                                                                                                       \
  "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"                     \
  "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"                   \
  "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"
#define JPEG_DHT_DC_CHROMA "00030101010101010101010000000000" "000102030405060708090a0b"
#define JPEG_DHT_AC_CHROMA                                                                                                                 \
  "00020102040403040705040400010277"                                                                                                       \
  "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"                   \
  "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"                 \
  "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"
// [0] DC luminance, [1] DC chrominance, [2] AC luminance, [3] AC chrominance
static __device__ const JpegHuffTab g_jpeg_huff[4] = {jpeg_make_huff(JPEG_DHT_DC_LUMA), jpeg_make_huff(JPEG_DHT_DC_CHROMA), jpeg_make_huff(JPEG_DHT_AC_LUMA),
                                                      jpeg_make_huff(JPEG_DHT_AC_CHROMA)};

// ------------------------------------------------------------------ geometry and the workspace
struct JpegPlan {
  int mcux, mcuy, nb;        // MCUs across / down, blocks per image (6 per MCU)
  int maxchunks, rawchunks;  // chunks an image's stream can have; chunks that are stored (those that can reach `cap`)
  size_t off_coef, off_bits, off_tot, off_ff, off_raw, bytes;
};
static inline size_t jpeg_round16(size_t b) { return (b + 15) & ~(size_t)15; }
static inline bool jpeg_plan(int N, int H, int W, int cap, JpegPlan& p) {
  if (N <= 0 || N > 65535 || H < 1 || W < 1 || H > JPEG_MAX_DIM || W > JPEG_MAX_DIM || cap < 1) return false;
  p.mcux = (W + 15) / 16;
  p.mcuy = (H + 15) / 16;
  p.nb = p.mcux * p.mcuy * 6;
  p.maxchunks = cdiv((long)p.nb * JPEG_BLOCK_MAX_BYTES, JPEG_CHUNK);
  const int capchunks = cdiv(cap, JPEG_CHUNK);
  p.rawchunks = capchunks < p.maxchunks ? capchunks : p.maxchunks;
  p.off_coef = 0;
  p.off_bits = p.off_coef + (size_t)N * p.nb * 128;
  p.off_tot = p.off_bits + jpeg_round16((size_t)N * p.nb * 4);
  p.off_ff = p.off_tot + jpeg_round16((size_t)N * 4);
  p.off_raw = p.off_ff + jpeg_round16((size_t)N * p.maxchunks * 4);
  p.bytes = p.off_raw + (size_t)N * p.rawchunks * JPEG_CHUNK;
  return true;
}

// ------------------------------------------------------------------ stage 1: coefficients
__device__ __forceinline__ int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// one pass of libjpeg's jfdctint.c (CONST_BITS 13, PASS1_BITS 2) over eight values: FIRST = the row pass
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct8(int (&d)[8]) {
  constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;  // round(c * 8192)
  constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;
  constexpr int NB = FIRST ? 11 : 15;
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = FIRST ? (t10 + t11) * 4 : jpeg_descale(t10 + t11, 2);
  d[4] = FIRST ? (t10 - t11) * 4 : jpeg_descale(t10 - t11, 2);
  const int y1 = (t12 + t13) * F_0_541;
  d[2] = jpeg_descale(y1 + t13 * F_0_765, NB);
  d[6] = jpeg_descale(y1 - t12 * F_1_847, NB);
  const int z5 = (t4 + t6 + t5 + t7) * F_1_175;
  const int z1 = -(t4 + t7) * F_0_899, z2 = -(t5 + t6) * F_2_562, z3 = -(t4 + t6) * F_1_961 + z5, z4 = -(t5 + t7) * F_0_390 + z5;
  d[7] = jpeg_descale(t4 * F_0_298 + z1 + z3, NB);
  d[5] = jpeg_descale(t5 * F_2_053 + z2 + z4, NB);
  d[3] = jpeg_descale(t6 * F_3_072 + z2 + z3, NB);
  d[1] = jpeg_descale(t7 * F_1_501 + z1 + z4, NB);
}

#define JPEG_STRIP_PIX 64                     // pixels across a workgroup's strip: four MCUs, one per wave
#define JPEG_STRIP_BYTES (JPEG_STRIP_PIX * 3)  // 192 = twelve 16-byte chunks per row
template <bool WIDE>  // WIDE: W % 16 == 0 and a 16-byte aligned image pointer: every row chunk of the strip is one aligned 16-byte load
__global__ __launch_bounds__(256) void jpeg_coef_kernel(const unsigned char* __restrict__ img, uint4* __restrict__ coef, int H, int W, int mcux, int nb,
                                                        int quality) {
  __shared__ uint4 rawv[16 * JPEG_STRIP_BYTES / 16];  // the strip's RGB bytes, rows clamped to H - 1
  __shared__ unsigned char ysm[4][16][16];
  __shared__ unsigned char csm[2][4][8][8];
  __shared__ int work[4][6][8][9];
  __shared__ uint4 outv[4 * 6 * 8];  // [wave][block][64] int16
  __shared__ int qdiv[2][64];
  __shared__ unsigned char zpos[64];
  unsigned char* raw = (unsigned char*)rawv;
  short* outc = (short*)outv;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = blockIdx.x * JPEG_STRIP_PIX, y0 = blockIdx.y * 16;
  const size_t n = blockIdx.z;
  const unsigned char* im = img + n * (size_t)H * W * 3;
  if (tid < 128) {  // jpeg_set_quality(quality, force_baseline): the divisor of jfdctint's scaled output is the table entry << 3
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    int q = ((int)g_jpeg_qbase[tid >> 6][tid & 63] * s + 50) / 100;
    q = q < 1 ? 1 : (q > 255 ? 255 : q);
    qdiv[tid >> 6][tid & 63] = q << 3;
  } else if (tid < 192) {
    zpos[tid - 128] = g_jpeg_zigzag.pos[tid - 128];
  }
  if constexpr (WIDE) {
    if (tid < 16 * 12) {
      const int r = tid / 12, c = tid - r * 12;
      const int yy = y0 + r < H ? y0 + r : H - 1;
      const long xb = (long)x0 * 3 + c * 16;
      if (xb < (long)W * 3) rawv[tid] = *(const uint4*)(im + (size_t)yy * W * 3 + xb);  // W * 3 is a multiple of 16: a chunk is wholly inside the row or wholly outside
    }
  } else {
    // any width, any alignment (W % 16 == 0 on an aligned pointer, the samplers' case, is the hot path above): a thread owns one byte column of the strip, so a
    // wave's load is 64 consecutive bytes of a row, and its pixel and channel are worked out once, not per byte
    if (tid < JPEG_STRIP_BYTES) {
      const int px = tid / 3, chn = tid - px * 3;
      const int xx = x0 + px < W ? x0 + px : W - 1;
      const unsigned char* col = im + (size_t)xx * 3 + chn;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int yy = y0 + r < H ? y0 + r : H - 1;
        raw[r * JPEG_STRIP_BYTES + tid] = col[(size_t)yy * W * 3];
      }
    }
  }
  __syncthreads();
  const int mx = blockIdx.x * 4 + wave;  // this wave's MCU
  const bool live = mx < mcux;
  // chroma rows exist up to the even height only: rows of down-sampled chroma beyond that repeat the last one (libjpeg pads AFTER down-sampling)
  const int cy_last = ((H + (H & 1)) >> 1) - 1 - (y0 >> 1);  // last computed chroma row of this strip, >= 0
  if (live) {
    const int qy = lane >> 3, qx = lane & 7;
    int cb = 0, cr = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        int lx = wave * 16 + 2 * qx + dx;
        if (x0 + lx > W - 1) lx = W - 1 - x0;  // columns replicate the last pixel
        const unsigned char* p = raw + (2 * qy + dy) * JPEG_STRIP_BYTES + lx * 3;
        const int R = p[0], G = p[1], B = p[2];
        ysm[wave][2 * qy + dy][2 * qx + dx] = (unsigned char)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
        cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
        cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
      }
    const int bias = 1 + (qx & 1);  // 1, 2, 1, 2, ... along the output row (an MCU starts at an even chroma column)
    csm[0][wave][qy][qx] = (unsigned char)((cb + bias) >> 2);
    csm[1][wave][qy][qx] = (unsigned char)((cr + bias) >> 2);
  }
  __syncthreads();
  const int blk = lane >> 3, rc = lane & 7;  // lanes 0..47: (block, row) in the row pass, (block, column) in the column pass
  if (live && blk < 6) {
    int d[8];
    if (blk < 4) {
      const unsigned char* p = &ysm[wave][(blk >> 1) * 8 + rc][(blk & 1) * 8];
#pragma unroll
      for (int i = 0; i < 8; ++i) d[i] = (int)p[i] - 128;
    } else {
      const unsigned char* p = &csm[blk - 4][wave][rc < cy_last ? rc : cy_last][0];
#pragma unroll
      for (int i = 0; i < 8; ++i) d[i] = (int)p[i] - 128;
    }
    jpeg_fdct8<true>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) work[wave][blk][rc][i] = d[i];
  }
  __syncthreads();
  // a Y block that starts at or beyond the image rounded up to 8 is a dummy block: all AC zero, DC = the DC of the block before it in the MCU
  const int Wr = (W + 7) & ~7, Hr = (H + 7) & ~7;
  if (live && blk < 6) {
    const bool dummy = blk < 4 && (mx * 16 + (blk & 1) * 8 >= Wr || y0 + (blk >> 1) * 8 >= Hr);
    int d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = work[wave][blk][i][rc];
    jpeg_fdct8<false>(d);
    short* o = outc + (wave * 6 + blk) * 64;
    const int* qd = qdiv[blk >= 4];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = i * 8 + rc, dv = qd[k];
      const int a = d[i] < 0 ? -d[i] : d[i];
      const int q = (a + (dv >> 1)) / dv;  // truncating division of the magnitude, then the sign
      o[zpos[k]] = dummy ? (short)0 : (short)(d[i] < 0 ? -q : q);
    }
  }
  __syncthreads();
  if (live && lane == 0) {
    short* o = outc + wave * 6 * 64;
    for (int k = 1; k < 4; ++k)
      if (mx * 16 + (k & 1) * 8 >= Wr || y0 + (k >> 1) * 8 >= Hr) o[k * 64] = o[(k - 1) * 64];
  }
  __syncthreads();
  if (live && lane < 48) {
    const size_t mcu = (size_t)blockIdx.y * mcux + mx;
    coef[(n * nb + mcu * 6) * 8 + lane] = outv[wave * 48 + lane];
  }
}

// ------------------------------------------------------------------ the Huffman coder of one block, shared by the counting and the packing stage
struct JpegHuffLds {
  unsigned int dc[2][16];
  unsigned int ac[2][256];
};
__device__ __forceinline__ void jpeg_stage_huff(JpegHuffLds& h) {  // the caller synchronises
  for (int e = threadIdx.x; e < 512; e += blockDim.x) h.ac[e >> 8][e & 255] = g_jpeg_huff[2 + (e >> 8)].e[e & 255];
  if (threadIdx.x < 32) h.dc[threadIdx.x >> 4][threadIdx.x & 15] = g_jpeg_huff[threadIdx.x >> 4].e[threadIdx.x & 15];
}
// a value's code: Huffman code of (run, size category), then `size` low bits of the value (value - 1 for negatives)
template <class Sink>
__device__ __forceinline__ void jpeg_put_value(Sink& sink, const unsigned int* tab, int run, int v) {
  const int a = v < 0 ? -v : v;
  const int s = a ? 32 - __clz(a) : 0;
  // every (run, s) asked for has a code: 8-bit samples through this FDCT and divisors >= 8 give |AC| <= 1023 (s <= 10) and |DC difference| <= 2047 (s <= 11)
  const unsigned e = tab[run << 4 | s];
  const unsigned low = (unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
  sink.put((e & 0xffffu) << s | low, (int)(e >> 16) + s);
}
// block b of an image whose coefficients start at `c` (eight uint4 per block): DC difference against the previous block of the same component in scan order
// (dummy blocks take part), AC run/size with ZRL and EOB
template <class Sink>
__device__ __forceinline__ void jpeg_code_block(const uint4* __restrict__ c, int b, const JpegHuffLds& h, Sink& sink) {
  const short* cs = (const short*)c;
  const int k = b % 6, chroma = k >= 4;
  int pred = 0;
  if (k >= 1 && k <= 3) pred = cs[(size_t)(b - 1) * 64];
  else if (b >= 6) pred = cs[(size_t)(b - (k == 0 ? 3 : 6)) * 64];
  const unsigned int* ac = h.ac[chroma];
  int run = 0;
  for (int j = 0; j < 8; ++j) {
    const uint4 v4 = c[(size_t)b * 8 + j];
    const unsigned w[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int v = (int)(short)(w[i >> 1] >> ((i & 1) * 16));
      if (j == 0 && i == 0) {
        jpeg_put_value(sink, h.dc[chroma], 0, v - pred);
        continue;
      }
      if (v == 0) {
        ++run;
        continue;
      }
      while (run > 15) {
        sink.put(ac[0xF0] & 0xffffu, (int)(ac[0xF0] >> 16));
        run -= 16;
      }
      jpeg_put_value(sink, ac, run, v);
      run = 0;
    }
  }
  if (run) sink.put(ac[0] & 0xffffu, (int)(ac[0] >> 16));
}

struct JpegCountSink {
  unsigned bits;
  __device__ __forceinline__ void put(unsigned, int n) { bits += (unsigned)n; }
};
// ORs codes into a window of JPEG_CHUNK_WORDS words of the stream (bit p of the stream is bit 31 - p % 32 of word p / 32: big-endian words); `pos` is the next
// bit relative to the window's start and may lie before or beyond it -- a block that straddles a chunk border is coded by both chunks, each keeps its part
struct JpegDepositSink {
  unsigned int* words;
  int pos;
  __device__ __forceinline__ void put(unsigned v, int n) {  // n <= 27
    const int wi = pos >> 5, sh = pos & 31;
    const unsigned long long x = (unsigned long long)v << (64 - n - sh);
    const unsigned hi = (unsigned)(x >> 32), lo = (unsigned)x;
    if ((unsigned)wi < (unsigned)JPEG_CHUNK_WORDS && hi) atomicOr(&words[wi], hi);
    if ((unsigned)(wi + 1) < (unsigned)JPEG_CHUNK_WORDS && lo) atomicOr(&words[wi + 1], lo);
    pos += n;
  }
};

// exclusive scan of one value per thread over a 256-thread workgroup; sm: four words; every thread gets the workgroup's total
__device__ __forceinline__ unsigned jpeg_block_scan(unsigned v, unsigned* sm, unsigned& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();  // the previous use of sm is over
  if (lane == 63) sm[wv] = inc;
  __syncthreads();
  unsigned base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned s = sm[i];
    base += i < wv ? s : 0u;
    total += s;
  }
  return base + inc - v;
}

// ------------------------------------------------------------------ stage 2: bits per block
__global__ __launch_bounds__(256) void jpeg_bits_kernel(const uint4* __restrict__ coef, unsigned* __restrict__ bits, int nb, size_t total) {
  __shared__ JpegHuffLds h;
  jpeg_stage_huff(h);
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t n = i / nb;
  const int b = (int)(i - n * nb);
  JpegCountSink sink{0};
  jpeg_code_block(coef + n * nb * 8, b, h, sink);
  bits[i] = sink.bits;
}

// ------------------------------------------------------------------ stage 3: bit offsets (one workgroup per image, tiles of 256 with a carry: any block count)
__global__ __launch_bounds__(256) void jpeg_scan_bits_kernel(unsigned* __restrict__ bits, unsigned* __restrict__ tot, int nb) {
  __shared__ unsigned sm[4];
  unsigned* p = bits + (size_t)blockIdx.x * nb;
  unsigned carry = 0;
  for (int base = 0; base < nb; base += 256) {
    const int i = base + threadIdx.x;
    const unsigned v = i < nb ? p[i] : 0u;
    unsigned total;
    const unsigned e = jpeg_block_scan(v, sm, total);
    if (i < nb) p[i] = carry + e;
    carry += total;
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

__device__ __forceinline__ int jpeg_count_ff(unsigned w0, unsigned w1, long first, long rawbytes) {  // 0xFF bytes among the stream bytes first .. first + 7 that exist
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const unsigned b = ((k < 4 ? w0 : w1) >> (24 - 8 * (k & 3))) & 0xffu;
    cnt += (first + k < rawbytes && b == 0xffu) ? 1 : 0;
  }
  return cnt;
}

// ------------------------------------------------------------------ stage 4: the stream, chunk by chunk
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const uint4* __restrict__ coef, const unsigned* __restrict__ off, const unsigned* __restrict__ tot,
                                                        unsigned* __restrict__ ff, unsigned* __restrict__ rawbuf, int nb, int maxchunks, int rawchunks) {
  __shared__ JpegHuffLds h;
  __shared__ unsigned words[JPEG_CHUNK_WORDS];
  __shared__ unsigned sm[4];
  const int tid = threadIdx.x;
  const size_t n = blockIdx.y;
  jpeg_stage_huff(h);
  const uint4* c = coef + n * nb * 8;
  const unsigned* o = off + n * nb;
  const unsigned totalbits = tot[n];
  const long rawbytes = ((long)totalbits + 7) >> 3;
  long nch = (rawbytes + JPEG_CHUNK - 1) / JPEG_CHUNK;
  if (nch > maxchunks) nch = maxchunks;  // cannot happen (JPEG_BLOCK_MAX_BYTES); keeps every index inside the workspace regardless
  for (long ch = blockIdx.x; ch < nch; ch += gridDim.x) {
    __syncthreads();  // the previous chunk's words are read, the tables are staged
    words[tid] = 0u;
    words[tid + 256] = 0u;
    __syncthreads();
    const unsigned start = (unsigned)ch * (JPEG_CHUNK * 8), end = start + JPEG_CHUNK * 8;
    int lo = 0, hi = nb - 1;  // the last block that starts at or before the chunk (offsets increase strictly: every block has at least 4 bits)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (o[mid] <= start) lo = mid;
      else hi = mid - 1;
    }
    for (int b = lo + tid; b < nb; b += 256) {
      const unsigned ob = o[b];
      if (ob >= end) break;
      JpegDepositSink sink{words, (int)ob - (int)start};
      jpeg_code_block(c, b, h, sink);
    }
    __syncthreads();
    if (tid == 0 && (rawbytes - 1) / JPEG_CHUNK == ch && (totalbits & 7u)) {  // the last byte is padded with 1-bits
      const unsigned rel = totalbits - start, npad = 8u - (totalbits & 7u);
      words[rel >> 5] |= ((1u << npad) - 1u) << (32u - (rel & 31u) - npad);
    }
    __syncthreads();
    const unsigned w0 = words[2 * tid], w1 = words[2 * tid + 1];
    if (ch < rawchunks) *(uint2*)(rawbuf + ((n * rawchunks + ch) * JPEG_CHUNK_WORDS + 2 * tid)) = make_uint2(w0, w1);
    unsigned total;
    (void)jpeg_block_scan((unsigned)jpeg_count_ff(w0, w1, ch * JPEG_CHUNK + 8 * tid, rawbytes), sm, total);
    if (tid == 0) ff[n * maxchunks + ch] = total;
  }
}

// ------------------------------------------------------------------ stage 5: where every chunk's stuffed bytes start; the length
__global__ __launch_bounds__(256) void jpeg_scan_ff_kernel(unsigned* __restrict__ ff, const unsigned* __restrict__ tot, int* __restrict__ lengths,
                                                           int maxchunks) {
  __shared__ unsigned sm[4];
  unsigned* p = ff + (size_t)blockIdx.x * maxchunks;
  const long rawbytes = ((long)tot[blockIdx.x] + 7) >> 3;
  long nch = (rawbytes + JPEG_CHUNK - 1) / JPEG_CHUNK;
  if (nch > maxchunks) nch = maxchunks;
  unsigned carry = 0;
  for (int base = 0; base < nch; base += 256) {
    const int i = base + threadIdx.x;
    const unsigned v = i < nch ? p[i] : 0u;
    unsigned total;
    const unsigned e = jpeg_block_scan(v, sm, total);
    if (i < nch) p[i] = carry + e;
    carry += total;
  }
  if (threadIdx.x == 0) lengths[blockIdx.x] = (int)(rawbytes + carry + 2);  // < 2^31: at most 2 x 216 bytes x 393216 blocks
}

// ------------------------------------------------------------------ stage 6: the stuffed copy
__global__ __launch_bounds__(256) void jpeg_stuff_kernel(const unsigned* __restrict__ rawbuf, const unsigned* __restrict__ ffoff,
                                                         const unsigned* __restrict__ tot, unsigned char* __restrict__ out, int cap, int maxchunks,
                                                         int rawchunks) {
  __shared__ unsigned sm[4];
  const int tid = threadIdx.x;
  const size_t n = blockIdx.y;
  const long rawbytes = ((long)tot[n] + 7) >> 3;
  long nch = (rawbytes + JPEG_CHUNK - 1) / JPEG_CHUNK;
  if (nch > rawchunks) nch = rawchunks;  // rawchunks <= maxchunks; a chunk that was not stored starts at or beyond cap
  unsigned char* o = out + n * (size_t)cap;
  for (long ch = blockIdx.x; ch < nch; ch += gridDim.x) {
    const uint2 w = *(const uint2*)(rawbuf + ((n * rawchunks + ch) * JPEG_CHUNK_WORDS + 2 * tid));
    const long first = ch * JPEG_CHUNK + 8 * tid;
    unsigned total;
    const unsigned before = jpeg_block_scan((unsigned)jpeg_count_ff(w.x, w.y, first, rawbytes), sm, total);
    long pos = first + ffoff[n * maxchunks + ch] + before;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (first + k >= rawbytes) break;
      const unsigned b = ((k < 4 ? w.x : w.y) >> (24 - 8 * (k & 3))) & 0xffu;
      if (pos < cap) o[pos] = (unsigned char)b;
      ++pos;
      if (b == 0xffu) {
        if (pos < cap) o[pos] = 0;
        ++pos;
      }
      if (first + k == rawbytes - 1) {  // EOI
        if (pos < cap) o[pos] = 0xff;
        if (pos + 1 < cap) o[pos + 1] = 0xd9;
      }
    }
  }
}

// ------------------------------------------------------------------ the C entry points
extern "C" size_t lfm_jpeg_encode_workspace_bytes(int N, int H, int W, int cap) {
  JpegPlan p;
  return jpeg_plan(N, H, W, cap, p) ? p.bytes : 0;
}

extern "C" int lfm_jpeg_encode_rgb8(const uint8_t* img_nhwc, int N, int H, int W, int quality, int cap, void* workspace, size_t workspace_bytes,
                                    uint8_t* out, int32_t* lengths, lfm_stream_t stream) {
  if (!img_nhwc || !workspace || !out || !lengths || quality < 1 || quality > 100) return LFM_ERR_ARG;
  JpegPlan p;
  if (!jpeg_plan(N, H, W, cap, p)) return LFM_ERR_SHAPE;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)lengths & 3)) return LFM_ERR_ALIGN;
  if (workspace_bytes < p.bytes) return LFM_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint4* coef = (uint4*)(ws + p.off_coef);
  unsigned* bits = (unsigned*)(ws + p.off_bits);
  unsigned* tot = (unsigned*)(ws + p.off_tot);
  unsigned* ff = (unsigned*)(ws + p.off_ff);
  unsigned* raw = (unsigned*)(ws + p.off_raw);
  const dim3 cgrid(cdiv(p.mcux, 4), p.mcuy, N);
  if (W % 16 == 0 && !((uintptr_t)img_nhwc & 15))
    hipLaunchKernelGGL(jpeg_coef_kernel<true>, cgrid, dim3(256), 0, st, img_nhwc, coef, H, W, p.mcux, p.nb, quality);
  else
    hipLaunchKernelGGL(jpeg_coef_kernel<false>, cgrid, dim3(256), 0, st, img_nhwc, coef, H, W, p.mcux, p.nb, quality);
  LFM_CHECK_LAUNCH();
  const size_t blocks = (size_t)N * p.nb;
  hipLaunchKernelGGL(jpeg_bits_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, coef, bits, p.nb, blocks);
  LFM_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_scan_bits_kernel, dim3(N), dim3(256), 0, st, bits, tot, p.nb);
  LFM_CHECK_LAUNCH();
  // workgroups per image of the chunk kernels: about 2048 in all (8 per CU), never more than the image can have chunks; each strides over its image's chunks
  int per = 2048 / N;
  per = per < 1 ? 1 : (per > p.maxchunks ? p.maxchunks : per);
  hipLaunchKernelGGL(jpeg_pack_kernel, dim3(per, N), dim3(256), 0, st, coef, bits, tot, ff, raw, p.nb, p.maxchunks, p.rawchunks);
  LFM_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_scan_ff_kernel, dim3(N), dim3(256), 0, st, ff, tot, lengths, p.maxchunks);
  LFM_CHECK_LAUNCH();
  const int sper = per > p.rawchunks ? p.rawchunks : per;
  hipLaunchKernelGGL(jpeg_stuff_kernel, dim3(sper, N), dim3(256), 0, st, raw, ff, tot, out, cap, p.maxchunks, p.rawchunks);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}
