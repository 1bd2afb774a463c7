// srsran_4g_amd/csrc/ldpc_api.cpp -- C-ABI host side of the HIP NR LDPC decoder.
//
// Implements include/srsran_ldpc.h (the srsran_ldpc_decoder_* surface of
// lib/include/srsran/phy/fec/ldpc/ldpc_decoder.h and create_compact_pcm of base_graph.h) over
// ldpc_kernel.hip.  Host semantics follow ldpc_decoder.c:
//   init (args check, geometry, compact PCM, default 10 iterations)   ldpc_decoder.c:552-648
//   rate-matched length clamp -> number of layers                     ldpc_decoder.c:48-70
//   return values (max_nof_iter / iterations until CRC / 0)           ldpc_decoder.c:72-95
// The transmit side (srsran_ldpc_encoder_*, srsran_ldpc_rm_tx*) runs over ldpc_enc_kernel.hip:
//   encoder init (geometry, compact PCM, high-rate case)               ldpc_encoder.c:99-134, 511-569
//   length rules of encode_rm -> rows computed                         ldpc_encoder.c:59-92
//   rate matcher checks, k0 / Ncb                                      ldpc_rm.c:113-167, 582-610
// There is no CPU fallback: without a HIP device init fails with SRSRAN_ERROR.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/srsran_ldpc.h"
#include "dev_buf.h"
#include "ldpc_enc_kernel.h"
#include "ldpc_internal.h"

#include "ldpc_bg_tables.inc"

using namespace srsran_amd;

namespace {

struct Graph {
  int                   M, N, K, ne;
  const unsigned short* rs;
  const unsigned char*  col;
  const unsigned short* V;  // this lifting size's set
};

// 38.212 Table 5.3.2-1: Z = a * 2^j, set index by a
int ls_index(int ls)
{
  static const int A[8] = {2, 3, 5, 7, 9, 11, 13, 15};
  if (ls < 2 || ls > MAX_LIFTSIZE) {
    return -1;
  }
  for (int i = 0; i < 8; i++) {
    int z = A[i];
    while (z < ls) {
      z *= 2;
    }
    if (z == ls) {
      return i;
    }
  }
  return -1;
}

bool graph(int bg, int ls, Graph& g)
{
  const int set = ls_index(ls);
  if (set < 0 || (bg != BG1 && bg != BG2)) {
    return false;
  }
  g.M   = bg == BG1 ? BG1M : BG2M;
  g.N   = bg == BG1 ? BG1Nfull : BG2Nfull;
  g.K   = g.N - g.M;
  g.rs  = bg == BG1 ? LDPC_BG1_ROW_START : LDPC_BG2_ROW_START;
  g.col = bg == BG1 ? LDPC_BG1_COL : LDPC_BG2_COL;
  g.V   = bg == BG1 ? LDPC_BG1_V[set] : LDPC_BG2_V[set];
  g.ne  = g.rs[g.M];
  return true;
}

// V mod ls per edge, edge order: the table the decoder and the encoder kernels read
std::vector<uint32_t> shift_table(const Graph& g, int ls)
{
  std::vector<uint32_t> sh(g.ne);
  for (int e = 0; e < g.ne; e++) {
    sh[e] = (uint32_t)(g.V[e] % ls);
  }
  return sh;
}

struct Ctx {
  hipStream_t stream    = nullptr;
  DevBuf<uint32_t> d_sh;
  DevBuf<int8_t>   d_in;   // single-codeword staging of the host-synchronous calls
  DevBuf<uint8_t>  d_out;
  DevBuf<uint8_t>  d_ret;
  DevBuf<uint8_t>  d_lut;  // scale(m), m = 0..127
  int         bits       = 8;  // LLR / message width: 8 (C, C_AVX2, C_AVX512) or 16 (S)
  int         scale_mode = LDPC_SCALE_SIMD;
  int         sf         = 0;
  std::map<uint64_t, DevBuf<uint32_t>> xpow;  // (poly, order) -> x^n mod P, n = 0 .. liftK
};

// x^n mod P for n = 0 .. nmax (P with its x^order bit)
std::vector<uint32_t> xpow_table(uint32_t poly, int order, int nmax)
{
  std::vector<uint32_t> t(nmax + 1);
  uint32_t              v    = 1;
  const uint32_t        mask = (1u << order) - 1u;
  for (int n = 0; n <= nmax; n++) {
    t[n] = v;
    v    = (v & (1u << (order - 1))) ? ((v << 1) ^ poly) : (v << 1);
    v &= mask;
  }
  return t;
}

void free_ctx(Ctx* c)
{
  if (!c) {
    return;
  }
  if (c->stream) {
    hipStreamSynchronize(c->stream);  // the buffers go with `delete c`, after the stream
    hipStreamDestroy(c->stream);
  }
  delete c;
}

void free_dec(void* o)
{
  srsran_ldpc_decoder_t* q = static_cast<srsran_ldpc_decoder_t*>(o);
  free_ctx(static_cast<Ctx*>(q->ptr));
  free(q->pcm);
  free(q->var_indices);
}

const uint32_t* xpow_for(srsran_ldpc_decoder_t* q, const srsran_crc_t* crc)
{
  Ctx*           c   = static_cast<Ctx*>(q->ptr);
  const uint64_t key = ((uint64_t)(uint32_t)crc->polynom << 8) | (uint32_t)crc->order;
  auto           it  = c->xpow.find(key);
  if (it != c->xpow.end()) {
    return it->second;
  }
  const auto t = xpow_table((uint32_t)crc->polynom, crc->order, q->liftK);
  DevBuf<uint32_t> d;
  if (!d.reserve(t.size()) || hipMemcpy(d, t.data(), t.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    return nullptr;
  }
  return c->xpow[key] = std::move(d);
}

// ldpc_decoder.c:48-70: clamp the rate-matched length and derive the processed layers
int layers_for(const srsran_ldpc_decoder_t* q, uint32_t len)
{
  if (len > (uint32_t)q->liftN - 2u * q->ls) {
    len = q->liftN - 2u * q->ls;
  }
  if (len < (uint32_t)(q->bgK + 2) * q->ls) {
    len = (uint32_t)(q->bgK + 2) * q->ls;
  }
  if (len % q->ls) {
    len = (len / q->ls + 1) * q->ls;
  }
  return (int)(len / q->ls) - q->bgK + 2;
}

// llr_stride in bytes; bits = width of the caller's LLRs (must match the decoder type)
int launch(srsran_ldpc_decoder_t* q, const void* d_llrs, int bits, uint32_t llr_stride, uint32_t nof_cw,
           uint32_t len, const srsran_crc_t* crc, uint8_t* d_message, uint32_t message_stride, int packed,
           uint8_t* d_ret, hipStream_t stream)
{
  Ctx* c = static_cast<Ctx*>(q->ptr);
  if (!c || !d_llrs || !d_message) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (bits != c->bits) {
    fprintf(stderr, "[srsran_4g_amd] LDPC: %d-bit LLRs given to a %d-bit decoder\n", bits, c->bits);
    return SRSRAN_ERROR;
  }
  if (crc && (crc->order != 16 && crc->order != 24)) {
    fprintf(stderr, "[srsran_4g_amd] LDPC: CRC order %d not supported\n", crc->order);
    return SRSRAN_ERROR;
  }
  if (packed && (q->liftK % 8)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  LdpcArgs a;
  memset(&a, 0, sizeof(a));
  a.in         = d_llrs;
  a.llr_bits   = bits;
  a.in_stride  = llr_stride;
  a.out        = d_message;
  a.out_stride = message_stride;
  a.out_packed = packed;
  a.ret        = d_ret;
  a.ncw        = nof_cw;
  a.ls         = q->ls;
  a.cw_per_wg  = ldpc_cw_per_wg(q->ls, bits);
  a.n_layers   = layers_for(q, len);
  a.max_iter   = (int)q->max_nof_iter;
  a.scale_mode = c->scale_mode;
  a.sf         = c->sf;
  a.sh         = c->d_sh;
  a.scale_lut  = c->d_lut;
  a.magic_ls   = (uint32_t)((0x100000000ull + q->ls - 1) / q->ls);
  if (crc) {
    a.xpow = xpow_for(q, crc);
    if (!a.xpow) {
      return SRSRAN_ERROR;
    }
    a.crc_poly  = (uint32_t)crc->polynom;
    a.crc_order = crc->order;
  }
  return ldpc_launch(q->bg == BG1 ? 0 : 1, a, stream) == hipSuccess ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}

int decode_impl(srsran_ldpc_decoder_t* q, const void* llrs, int bits, uint8_t* message, uint32_t len,
                const srsran_crc_t* crc)
{
  Ctx* c = static_cast<Ctx*>(q->ptr);
  if (!c || !llrs || !message) {
    return SRSRAN_ERROR;
  }
  const size_t n = ((size_t)q->liftN - 2u * q->ls) * (size_t)(bits / 8);
  if (bits != c->bits || hipMemcpyAsync(c->d_in, llrs, n, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  if (launch(q, c->d_in, bits, (uint32_t)n, 1, len, crc, c->d_out, q->liftK, 0, c->d_ret, c->stream) !=
      SRSRAN_SUCCESS) {
    return SRSRAN_ERROR;
  }
  uint8_t ret = 0;
  if (hipMemcpyAsync(message, c->d_out, q->liftK, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipMemcpyAsync(&ret, c->d_ret, 1, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  return (int)ret;
}

int decode_c_impl(void* o, const int8_t* llrs, uint8_t* message, uint32_t len, srsran_crc_t* crc)
{
  return decode_impl(static_cast<srsran_ldpc_decoder_t*>(o), llrs, 8, message, len, crc);
}

int decode_s_impl(void* o, const int16_t* llrs, uint8_t* message, uint32_t len, srsran_crc_t* crc)
{
  return decode_impl(static_cast<srsran_ldpc_decoder_t*>(o), llrs, 16, message, len, crc);
}


// ---- transmit side ----
struct EncCtx {
  hipStream_t      stream = nullptr;
  DevBuf<uint32_t> d_sh;
  DevBuf<uint8_t>  d_in;  // single-codeword staging of the host-synchronous calls
  DevBuf<uint8_t>  d_out;
  int              hr_case = 1;
};

void free_enc_ctx(EncCtx* c)
{
  if (!c) {
    return;
  }
  if (c->stream) {
    hipStreamSynchronize(c->stream);  // the buffers go with `delete c`, after the stream
    hipStreamDestroy(c->stream);
  }
  delete c;
}

void free_enc(void* o)
{
  srsran_ldpc_encoder_t* q = static_cast<srsran_ldpc_encoder_t*>(o);
  free_enc_ctx(static_cast<EncCtx*>(q->ptr));
  free(q->pcm);
}

// ldpc_encoder.c:63-92: clamp the rate-matched length, raise it to the high-rate region, round it up to
// whole chunks; the base-graph rows that covers
int enc_rows_for(const srsran_ldpc_encoder_t* q, uint32_t len)
{
  if (len > (uint32_t)q->liftN - 2u * q->ls) {
    len = q->liftN - 2u * q->ls;
  }
  if (len < (uint32_t)(q->bgK + 2) * q->ls) {
    len = (uint32_t)(q->bgK + 2) * q->ls;
  }
  if (len % q->ls) {
    len = (len / q->ls + 1) * q->ls;
  }
  return (int)(len / q->ls) - q->bgK + 2;
}

int enc_launch(srsran_ldpc_encoder_t* q, const uint8_t* d_msg, uint32_t msg_stride, uint32_t nof_cw, uint32_t len,
               uint8_t* d_cw, uint32_t cw_stride, hipStream_t stream)
{
  EncCtx* c = static_cast<EncCtx*>(q->ptr);
  if (!c || !d_msg || !d_cw) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  LdpcEncArgs a;
  memset(&a, 0, sizeof(a));
  a.in         = d_msg;
  a.in_stride  = msg_stride;
  a.out        = d_cw;
  a.out_stride = cw_stride;
  a.ncw        = nof_cw;
  a.ls         = q->ls;
  a.hr_case    = c->hr_case;
  a.n_rows     = enc_rows_for(q, len);
  a.sh         = c->d_sh;
  a.magic_ls   = (uint32_t)((0x100000000ull + q->ls - 1) / q->ls);
  return ldpc_enc_launch(q->bg == BG1 ? 0 : 1, a, stream) == hipSuccess ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}

int encode_impl(void* o, const uint8_t* input, uint8_t* output, uint32_t input_length, uint32_t cdwd_rm_length)
{
  srsran_ldpc_encoder_t* q = static_cast<srsran_ldpc_encoder_t*>(o);
  EncCtx*                c = static_cast<EncCtx*>(q->ptr);
  if (!c || !input || !output) {
    return -1;
  }
  if (input_length / q->bgK != q->ls) {  // ldpc_encoder.c:59-62
    fprintf(stderr, "[srsran_4g_amd] LDPC encoder: dimension mismatch\n");
    return -1;
  }
  const size_t n = (size_t)(enc_rows_for(q, cdwd_rm_length) + q->bgK - 2) * q->ls;  // bytes the reference writes
  if (hipMemcpyAsync(c->d_in, input, q->liftK, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      enc_launch(q, c->d_in, q->liftK, 1, cdwd_rm_length, c->d_out, (uint32_t)n, c->stream) != SRSRAN_SUCCESS ||
      hipMemcpyAsync(output, c->d_out, n, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    return -1;
  }
  return 0;
}

struct RmTxCtx {
  hipStream_t     stream = nullptr;
  DevBuf<uint8_t> d_in, d_out;
};

constexpr uint32_t kRmMaxE = 273 * 13 * 12 * 8 * 4;  // MAXE, ldpc_rm.c:77

}  // namespace

namespace srsran_amd {

int ldpc_layers_for(const srsran_ldpc_decoder_t* q, uint32_t len) { return layers_for(q, len); }

std::vector<uint32_t> ldpc_xpow_table(uint32_t poly, int order, int nmax) { return xpow_table(poly, order, nmax); }

const uint32_t* ldpc_shift_table(const srsran_ldpc_decoder_t* q)
{
  const Ctx* c = static_cast<const Ctx*>(q ? q->ptr : nullptr);
  return c ? c->d_sh.get() : nullptr;
}

int ldpc_ls_set_index(int ls) { return ls_index(ls); }

int ldpc_launch_cws(srsran_ldpc_decoder_t* q, const LdpcCw* d_cws, uint32_t n, const uint32_t* const xpow3[3],
                    uint32_t max_layers, hipStream_t stream)
{
  Ctx* c = static_cast<Ctx*>(q ? q->ptr : nullptr);
  if (!c || c->bits != 8) {
    return SRSRAN_ERROR;
  }
  LdpcArgs a;
  memset(&a, 0, sizeof(a));
  a.llr_bits   = 8;
  a.ncw        = n;
  a.ls         = q->ls;
  a.cw_per_wg  = ldpc_cw_per_wg(q->ls, 8);
  a.n_layers   = (int)std::min<uint32_t>(max_layers ? max_layers : q->bgM, q->bgM);
  a.max_iter   = (int)q->max_nof_iter;
  a.scale_mode = c->scale_mode;
  a.sf         = c->sf;
  a.sh         = c->d_sh;
  a.scale_lut  = c->d_lut;
  a.magic_ls   = (uint32_t)((0x100000000ull + q->ls - 1) / q->ls);
  a.cws        = d_cws;
  for (int i = 0; i < 3; i++) {
    a.xpow3[i] = xpow3[i];
  }
  return ldpc_launch(q->bg == BG1 ? 0 : 1, a, stream) == hipSuccess ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}

}  // namespace srsran_amd

extern "C" {

int create_compact_pcm(uint16_t* pcm, int8_t (*positions)[MAX_CNCT], srsran_basegraph_t bg, uint16_t ls)
{
  Graph g;
  if (!pcm || !graph(bg, ls, g)) {
    fprintf(stderr, "[srsran_4g_amd] Invalid lifting size %d\n", ls);
    return SRSRAN_ERROR;
  }
  for (int i = 0; i < g.M * g.N; i++) {
    pcm[i] = NO_CNCT;
  }
  for (int i = 0; i < g.M; i++) {
    for (int e = g.rs[i]; e < g.rs[i + 1]; e++) {
      pcm[i * g.N + g.col[e]] = (uint16_t)(g.V[e] % ls);
    }
    if (positions) {
      for (int k = 0; k < MAX_CNCT; k++) {
        const int e     = g.rs[i] + k;
        positions[i][k] = e < g.rs[i + 1] ? (int8_t)g.col[e] : (int8_t)-1;
      }
    }
  }
  return SRSRAN_SUCCESS;
}

int srsran_ldpc_decoder_init(srsran_ldpc_decoder_t* q, const srsran_ldpc_decoder_args_t* args)
{
  if (!q || !args) {
    return SRSRAN_ERROR;
  }
  memset(q, 0, sizeof(*q));
  Graph g;
  if (!graph(args->bg, args->ls, g)) {
    fprintf(stderr, "[srsran_4g_amd] LDPC: invalid base graph %d / lifting size %d\n", (int)args->bg + 1, args->ls);
    return SRSRAN_ERROR;
  }
  const float s = args->scaling_fctr;
  if (!(s > 0.0f) || s > 1.0f) {  // ldpc_decoder.c:596-601
    fprintf(stderr, "[srsran_4g_amd] LDPC: scaling factor must be in (0, 1]\n");
    return SRSRAN_ERROR;
  }
  int scale_mode;
  int bits = 8;
  switch (args->type) {
    case SRSRAN_LDPC_DECODER_S:  // ldpc_dec_s.c: 16-bit LLRs, 15-bit messages, scaling m*s100/100
      scale_mode = LDPC_SCALE_C;
      bits       = 16;
      break;
    case SRSRAN_LDPC_DECODER_C:
      scale_mode = LDPC_SCALE_C;
      break;
    case SRSRAN_LDPC_DECODER_C_AVX2:
    case SRSRAN_LDPC_DECODER_C_AVX512:
      scale_mode = LDPC_SCALE_SIMD;
      break;
    default:
      fprintf(stderr, "[srsran_4g_amd] LDPC decoder type %d not provided on the GPU (layered C/AVX2/AVX512/S only)\n",
              (int)args->type);
      return SRSRAN_ERROR;
  }
  q->bg           = args->bg;
  q->ls           = args->ls;
  q->bgN          = (uint8_t)g.N;
  q->bgM          = (uint8_t)g.M;
  q->bgK          = (uint8_t)g.K;
  q->liftK        = (uint16_t)(g.K * args->ls);
  q->liftM        = (uint16_t)(g.M * args->ls);
  q->liftN        = (uint16_t)(g.N * args->ls);
  q->max_nof_iter = args->max_nof_iter == 0 ? 10 : args->max_nof_iter;
  q->scaling_fctr = s;
  q->pcm          = static_cast<uint16_t*>(malloc(sizeof(uint16_t) * g.M * g.N));
  q->var_indices  = static_cast<int8_t(*)[MAX_CNCT]>(malloc((size_t)g.M * MAX_CNCT));
  if (!q->pcm || !q->var_indices || create_compact_pcm(q->pcm, q->var_indices, q->bg, q->ls) != SRSRAN_SUCCESS) {
    free(q->pcm);
    free(q->var_indices);
    memset(q, 0, sizeof(*q));
    return SRSRAN_ERROR;
  }
  Ctx* c        = new Ctx;
  c->scale_mode = scale_mode;
  c->bits       = bits;
  // ldpc_dec_c_avx2.c:148 / ldpc_dec_c.c:149 (float arithmetic as the reference)
  c->sf = scale_mode == LDPC_SCALE_SIMD ? (int)(uint16_t)((s + 0.00001525879) * 65535) : (int)(s * 100);
  const std::vector<uint32_t> sh = shift_table(g, args->ls);
  uint8_t lut[128];
  for (int m = 0; m < 128; m++) {  // ldpc_dec_c.c:282 / _mm256_scalei_epi8 (ldpc_dec_c_avx2.c:520-531)
    lut[m] = (uint8_t)(scale_mode == LDPC_SCALE_SIMD ? ((uint32_t)m * (uint32_t)c->sf) >> 16 : m * c->sf / 100);
  }
  const size_t n = ((size_t)q->liftN - 2u * q->ls) * (size_t)(bits / 8);
  if (!c->d_lut.reserve(128) || hipMemcpy(c->d_lut, lut, 128, hipMemcpyHostToDevice) != hipSuccess ||
      hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      !c->d_sh.reserve(sh.size()) || !c->d_in.reserve(n) || !c->d_out.reserve(q->liftK) || !c->d_ret.reserve(64) ||
      hipMemcpy(c->d_sh, sh.data(), sh.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    fprintf(stderr, "[srsran_4g_amd] LDPC: no HIP device / allocation failed\n");
    (void)hipGetLastError();
    free_ctx(c);
    free(q->pcm);
    free(q->var_indices);
    memset(q, 0, sizeof(*q));
    return SRSRAN_ERROR;
  }
  q->ptr  = c;
  q->free = free_dec;
  if (bits == 16) {
    q->decode_s = decode_s_impl;
  } else {
    q->decode_c = decode_c_impl;
  }
  return SRSRAN_SUCCESS;
}

void srsran_ldpc_decoder_free(srsran_ldpc_decoder_t* q)
{
  if (!q) {
    return;
  }
  if (q->free) {
    q->free(q);
  }
  memset(q, 0, sizeof(*q));
}

int srsran_ldpc_decoder_decode_f(srsran_ldpc_decoder_t* q, const float* llrs, uint8_t* message, uint32_t len)
{
  (void)q, (void)llrs, (void)message, (void)len;
  fprintf(stderr, "[srsran_4g_amd] LDPC: float decoder not provided on the GPU\n");
  return SRSRAN_ERROR;
}

int srsran_ldpc_decoder_decode_s(srsran_ldpc_decoder_t* q, const int16_t* llrs, uint8_t* message, uint32_t len)
{
  if (!q || !q->decode_s) {  // the reference calls a NULL decode_s for 8-bit decoder types
    fprintf(stderr, "[srsran_4g_amd] LDPC: decode_s needs a SRSRAN_LDPC_DECODER_S decoder\n");
    return SRSRAN_ERROR;
  }
  return q->decode_s(q, llrs, message, len, nullptr);
}

int srsran_ldpc_decoder_decode_c(srsran_ldpc_decoder_t* q, const int8_t* llrs, uint8_t* message, uint32_t len)
{
  if (!q || !q->decode_c) {
    return SRSRAN_ERROR;
  }
  return q->decode_c(q, llrs, message, len, nullptr);
}

int srsran_ldpc_decoder_decode_crc_c(srsran_ldpc_decoder_t* q,
                                     const int8_t*          llrs,
                                     uint8_t*               message,
                                     uint32_t               len,
                                     srsran_crc_t*          crc)
{
  if (!q || !q->decode_c) {
    return SRSRAN_ERROR;
  }
  return q->decode_c(q, llrs, message, len, crc);
}

int srsran_ldpc_decoder_gpu_decode_batch(srsran_ldpc_decoder_t* q,
                                         const int8_t*          d_llrs,
                                         uint32_t               llr_stride,
                                         uint32_t               nof_cw,
                                         uint32_t               cdwd_rm_length,
                                         const srsran_crc_t*    crc,
                                         uint8_t*               d_message,
                                         uint32_t               message_stride,
                                         int                    packed,
                                         uint8_t*               d_ret,
                                         void*                  stream)
{
  if (!q || !q->ptr) {
    return SRSRAN_ERROR;
  }
  return launch(q, d_llrs, 8, llr_stride, nof_cw, cdwd_rm_length, crc, d_message, message_stride, packed, d_ret,
                static_cast<hipStream_t>(stream));
}

int srsran_ldpc_decoder_gpu_decode_batch_s(srsran_ldpc_decoder_t* q,
                                           const int16_t*         d_llrs,
                                           uint32_t               llr_stride,
                                           uint32_t               nof_cw,
                                           uint32_t               cdwd_rm_length,
                                           const srsran_crc_t*    crc,
                                           uint8_t*               d_message,
                                           uint32_t               message_stride,
                                           int                    packed,
                                           uint8_t*               d_ret,
                                           void*                  stream)
{
  if (!q || !q->ptr) {
    return SRSRAN_ERROR;
  }
  return launch(q, d_llrs, 16, llr_stride * 2u, nof_cw, cdwd_rm_length, crc, d_message, message_stride, packed,
                d_ret, static_cast<hipStream_t>(stream));
}

int srsran_ldpc_encoder_init(srsran_ldpc_encoder_t* q, srsran_ldpc_encoder_type_t type, srsran_basegraph_t bg, uint16_t ls)
{
  if (!q) {
    return -1;
  }
  memset(q, 0, sizeof(*q));
  Graph g;
  if (!graph(bg, ls, g)) {
    fprintf(stderr, "[srsran_4g_amd] LDPC encoder: invalid base graph %d / lifting size %d\n", (int)bg + 1, ls);
    return -1;
  }
  if (type != SRSRAN_LDPC_ENCODER_C && type != SRSRAN_LDPC_ENCODER_AVX2 && type != SRSRAN_LDPC_ENCODER_AVX512) {
    fprintf(stderr, "[srsran_4g_amd] LDPC encoder: unknown type %d\n", (int)type);
    return -1;
  }
  q->bg    = bg;
  q->ls    = ls;
  q->bgN   = (uint8_t)g.N;
  q->bgM   = (uint8_t)g.M;
  q->bgK   = (uint8_t)g.K;
  q->liftK = (uint16_t)(g.K * ls);
  q->liftM = (uint16_t)(g.M * ls);
  q->liftN = (uint16_t)(g.N * ls);
  q->pcm   = static_cast<uint16_t*>(malloc(sizeof(uint16_t) * g.M * g.N));
  if (!q->pcm || create_compact_pcm(q->pcm, nullptr, bg, ls) != SRSRAN_SUCCESS) {
    free(q->pcm);
    memset(q, 0, sizeof(*q));
    return -1;
  }
  EncCtx*                     c  = new EncCtx;
  const std::vector<uint32_t> sh = shift_table(g, ls);
  c->hr_case                     = ldpc_enc_hr_case(bg == BG1 ? 0 : 1, ls_index(ls));
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || !c->d_sh.reserve(sh.size()) ||
      !c->d_in.reserve(q->liftK) || !c->d_out.reserve((size_t)q->liftN) ||
      hipMemcpy(c->d_sh, sh.data(), sh.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    fprintf(stderr, "[srsran_4g_amd] LDPC encoder: no HIP device / allocation failed\n");
    (void)hipGetLastError();
    free_enc_ctx(c);
    free(q->pcm);
    memset(q, 0, sizeof(*q));
    return -1;
  }
  q->ptr    = c;
  q->free   = free_enc;
  q->encode = encode_impl;
  return 0;
}

void srsran_ldpc_encoder_free(srsran_ldpc_encoder_t* q)
{
  if (!q) {
    return;
  }
  if (q->free) {
    q->free(q);
  }
  memset(q, 0, sizeof(*q));
}

int srsran_ldpc_encoder_encode(srsran_ldpc_encoder_t* q, const uint8_t* input, uint8_t* output, uint32_t input_length)
{
  if (!q || !q->encode) {
    return -1;
  }
  return q->encode(q, input, output, input_length, (uint32_t)q->liftN - 2u * q->ls);
}

int srsran_ldpc_encoder_encode_rm(srsran_ldpc_encoder_t* q,
                                  const uint8_t*         input,
                                  uint8_t*               output,
                                  uint32_t               input_length,
                                  uint32_t               cdwd_rm_length)
{
  if (!q || !q->encode) {
    return -1;
  }
  return q->encode(q, input, output, input_length, cdwd_rm_length);
}

int srsran_ldpc_encoder_gpu_encode_batch(srsran_ldpc_encoder_t* q,
                                         const uint8_t*         d_msg,
                                         uint32_t               msg_stride,
                                         uint32_t               nof_cw,
                                         uint32_t               cdwd_rm_length,
                                         uint8_t*               d_cw,
                                         uint32_t               cw_stride,
                                         void*                  stream)
{
  if (!q || !q->ptr) {
    return SRSRAN_ERROR;
  }
  return enc_launch(q, d_msg, msg_stride, nof_cw, cdwd_rm_length, d_cw, cw_stride, static_cast<hipStream_t>(stream));
}

int srsran_ldpc_rm_tx_init(srsran_ldpc_rm_t* p)
{
  if (!p) {
    return -1;
  }
  memset(p, 0, sizeof(*p));
  RmTxCtx* c = new RmTxCtx;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    fprintf(stderr, "[srsran_4g_amd] LDPC rate matcher: no HIP device\n");
    (void)hipGetLastError();
    delete c;
    return -1;
  }
  p->ptr = c;
  return 0;
}

void srsran_ldpc_rm_tx_free(srsran_ldpc_rm_t* q)
{
  if (!q) {
    return;
  }
  RmTxCtx* c = static_cast<RmTxCtx*>(q->ptr);
  if (c) {
    if (c->stream) {
      hipStreamSynchronize(c->stream);
      hipStreamDestroy(c->stream);
    }
    delete c;
  }
  q->ptr = nullptr;
}

int srsran_ldpc_rm_tx(srsran_ldpc_rm_t*        q,
                      const uint8_t*           input,
                      uint8_t*                 output,
                      const uint32_t           E,
                      const srsran_basegraph_t bg,
                      const uint32_t           ls,
                      const uint8_t            rv,
                      const srsran_mod_t       mod_type,
                      const uint32_t           Nref)
{
  RmTxCtx* c = static_cast<RmTxCtx*>(q ? q->ptr : nullptr);
  if (!c || !input || !output || (bg != BG1 && bg != BG2) || rv > 3) {
    return -1;
  }
  const uint32_t Qm = srsran_mod_bits_x_symbol(mod_type);
  if (E > kRmMaxE || Qm == 0 || E % Qm != 0) {  // init_rm, ldpc_rm.c:131-147
    fprintf(stderr, "[srsran_4g_amd] LDPC rate matcher: wrong E = %u for modulation order %u\n", E, Qm);
    return -1;
  }
  uint32_t k0, Ncb;
  nr_rm_tx_k0_ncb(bg == BG1 ? 0 : 1, ls, rv, Nref, &k0, &Ncb);
  q->N         = ls * (bg == BG1 ? 66u : 50u);
  q->E         = E;
  q->K         = ls * (bg == BG1 ? 22u : 10u);
  q->F         = 0;
  q->ls        = (uint16_t)ls;
  q->mod_order = Qm;
  q->bg        = bg;
  q->Ncb       = Ncb;
  q->k0        = k0;
  // the filler bytes (254) of an encoder's codeword form one range: find it, so that every output
  // bit has a closed-form source (bit_selection_rm_tx walks and tests every byte, ldpc_rm.c:185-192)
  uint32_t first = Ncb, last = 0, count = 0;
  for (uint32_t i = 0; i < Ncb; i++) {
    if (input[i] == 254) {
      first = count ? first : i;
      last  = i;
      count++;
    }
  }
  if (count && last - first + 1 != count) {
    fprintf(stderr, "[srsran_4g_amd] LDPC rate matcher: filler bits are not one range\n");
    return -1;
  }
  const NrRmTxSel sel = nr_rm_tx_sel(k0, Ncb, count ? first : Ncb, count ? last + 1 : Ncb);
  if (E == 0) {
    return 0;
  }
  if (sel.L == 0) {  // the reference's walk would never end
    return -1;
  }
  if (!c->d_in.reserve(Ncb) || !c->d_out.reserve(E) ||
      hipMemcpyAsync(c->d_in, input, Ncb, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      ldpc_rm_tx_launch(c->d_in, c->d_out, E, Qm, sel, c->stream) != hipSuccess ||
      hipMemcpyAsync(output, c->d_out, E, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    return -1;
  }
  return 0;
}

}  // extern "C"
