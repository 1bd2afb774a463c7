// tools/sch_host_check.cpp -- host-only check of csrc/fec_host.cpp and csrc/uci_host.cpp: the segmentation, the table
// CRC, the CQI reports, the UCI offset tables and the transmitter's UCI channel coding, none of which touches the GPU.
//
// Prints one line per case, the first word naming the kind:
//   cbsegm  tbs rc C K1 K2 K1_idx K2_idx C1 C2 F
//   crc     poly(hex) order nbits checksum(hex) data(hex, nbits / 8 bytes, '-' when empty)
//   cqi     type N L four pmi rank label2 | size | packed length | packed bits | the value's five words
//   beta    index beta_ack beta_cqi beta_harq beta_ri beta_cqi(table)  find_ack find_ri find_cqi of these three
//   find    which beta index
//   block   nin nout input-bits output-bits
//   cqilong nbits Q input-bits output-bits
// tests/test_sch_fec_host.py compares them with the oracle and with the compiled reference.  Every buffer a function
// reads or writes is a heap block of exactly the length it may touch, so the sanitizers' red zones catch one byte too
// many; the CQI round trip (pack, unpack, the same fields) is checked here.
//
// Build and run (no GPU):  c++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//     tools/sch_host_check.cpp srsran_4g_amd/csrc/fec_host.cpp srsran_4g_amd/csrc/uci_host.cpp -o /tmp/sch_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../srsran_4g_amd/csrc/uci_host.h"

using namespace srsran_amd;

namespace {

uint32_t g_lcg = 12345;
uint32_t rnd()
{
  g_lcg = g_lcg * 1664525u + 1013904223u;
  return g_lcg >> 8;
}

[[noreturn]] void fail(const char* what, int a, int b)
{
  fprintf(stderr, "FAIL %s: %d %d\n", what, a, b);
  exit(1);
}

void print_bits(const uint8_t* b, uint32_t n)
{
  for (uint32_t i = 0; i < n; i++) {
    if (b[i] > 1) {
      fail("not a bit", (int)i, b[i]);
    }
    putchar('0' + b[i]);
  }
  if (n == 0) {
    putchar('-');
  }
}

void segm()
{
  std::vector<uint32_t> list;
  for (uint32_t t = 0; t < 400000; t += 8 * 37) {  // tests/test_sch_host.py::test_cbsegm_matches_oracle's list
    list.push_back(t);
  }
  for (uint32_t t : {75376u, 97896u, 6120u, 6200u, 40u, 16u, 20u, 391656u, 500000u, 0u, 16u, 40u, 6120u, 6112u, 6128u,
                     391656u}) {
    list.push_back(t);
  }
  for (uint32_t tbs : list) {
    std::unique_ptr<srsran_cbsegm_t> s(new srsran_cbsegm_t);
    memset(s.get(), 0xA5, sizeof(*s));
    const int rc = srsran_cbsegm(s.get(), tbs);
    printf("cbsegm %u %d %u %u %u %u %u %u %u %u\n", tbs, rc, s->C, s->K1, s->K2, s->K1_idx, s->K2_idx, s->C1, s->C2,
           s->F);
  }
}

void crc()
{
  const struct {
    uint32_t poly;
    int      order;
  } polys[] = {{SRSRAN_LTE_CRC24A, 24}, {SRSRAN_LTE_CRC24B, 24}, {0x11021, 16}, {0x19B, 8}};
  for (auto p : polys) {
    for (int nbits : {1, 7, 8, 9, 64, 6144, 75400}) {
      const int                  n = nbits / 8;
      std::unique_ptr<uint8_t[]> d(new uint8_t[n]);  // exactly the bytes the checksum may read
      for (int i = 0; i < n; i++) {
        d[i] = (uint8_t)rnd();
      }
      srsran_crc_t h;
      if (srsran_crc_init(&h, p.poly, p.order)) {
        fail("srsran_crc_init", (int)p.poly, p.order);
      }
      const uint32_t c = srsran_crc_checksum_byte(&h, d.get(), nbits);
      printf("crc %x %d %d %x ", p.poly, p.order, nbits, c);
      for (int i = 0; i < n; i++) {
        printf("%02x", d[i]);
      }
      printf("%s\n", n ? "" : "-");
    }
  }
}

uint32_t mask(uint32_t v, uint32_t bits) { return bits >= 32 ? v : v & ((1u << bits) - 1); }

void cqi()
{
  const srsran_cqi_type_t types[] = {SRSRAN_CQI_TYPE_WIDEBAND, SRSRAN_CQI_TYPE_SUBBAND_UE,
                                     SRSRAN_CQI_TYPE_SUBBAND_UE_DIFF, SRSRAN_CQI_TYPE_SUBBAND_HL};
  for (srsran_cqi_type_t t : types) {
    for (int shape = 0; shape < (t == SRSRAN_CQI_TYPE_WIDEBAND ? 1 : 2); shape++) {
      for (int combo = 0; combo < 8; combo++) {
        srsran_cqi_cfg_t c;
        memset(&c, 0, sizeof(c));
        c.data_enable          = true;
        c.type                 = t;
        c.four_antenna_ports   = combo & 1;
        c.pmi_present          = combo & 2;
        c.rank_is_not_one      = combo & 4;
        c.N                    = shape ? 13 : 1;
        c.L                    = shape ? 6 : 2;
        c.subband_label_2_bits = shape != 0;
        const uint32_t wpmi    = c.four_antenna_ports ? 4 : c.rank_is_not_one ? 1 : 2;
        srsran_cqi_value_t v;
        memset(&v, 0, sizeof(v));
        switch (t) {
          case SRSRAN_CQI_TYPE_WIDEBAND:
            v.wideband.wideband_cqi     = (uint8_t)mask(rnd(), 4);
            v.wideband.spatial_diff_cqi = (uint8_t)mask(rnd(), 3);
            v.wideband.pmi              = (uint8_t)mask(rnd(), wpmi);
            break;
          case SRSRAN_CQI_TYPE_SUBBAND_UE:
            v.subband_ue.subband_cqi   = (uint8_t)mask(rnd(), 4);
            v.subband_ue.subband_label = (uint8_t)mask(rnd(), c.subband_label_2_bits ? 2 : 1);
            break;
          case SRSRAN_CQI_TYPE_SUBBAND_UE_DIFF:
            v.subband_ue_diff.wideband_cqi     = (uint8_t)mask(rnd(), 4);
            v.subband_ue_diff.subband_diff_cqi = (uint8_t)mask(rnd(), c.L);
            break;
          case SRSRAN_CQI_TYPE_SUBBAND_HL:
            v.subband_hl.wideband_cqi_cw0     = (uint8_t)mask(rnd(), 4);
            v.subband_hl.subband_diff_cqi_cw0 = mask(rnd() ^ (rnd() << 8), 2 * c.N);
            v.subband_hl.wideband_cqi_cw1     = (uint8_t)mask(rnd(), 4);
            v.subband_hl.subband_diff_cqi_cw1 = mask(rnd() ^ (rnd() << 8), 2 * c.N);
            v.subband_hl.pmi                  = mask(rnd(), wpmi);
            break;
        }
        const int size = srsran_cqi_size(&c);
        // exactly SRSRAN_CQI_MAX_BITS, as the prototype says: the largest report (61 + 3 bits) ends at its last byte
        std::unique_ptr<uint8_t[]> buf(new uint8_t[SRSRAN_CQI_MAX_BITS]);
        memset(buf.get(), 0, SRSRAN_CQI_MAX_BITS);
        const int n = srsran_cqi_value_pack(&c, &v, buf.get());
        if (n < 0 || n > SRSRAN_CQI_MAX_BITS) {
          fail("srsran_cqi_value_pack", (int)t, n);
        }
        srsran_cqi_value_t back;
        memset(&back, 0, sizeof(back));
        const int m = srsran_cqi_value_unpack(&c, buf.get(), &back);
        std::unique_ptr<uint8_t[]> again(new uint8_t[SRSRAN_CQI_MAX_BITS]);
        memset(again.get(), 0, SRSRAN_CQI_MAX_BITS);
        // the fields the report carries come back: packed again they give the same bits, and the words the report
        // does not carry stay zero
        if (srsran_cqi_value_pack(&c, &back, again.get()) != n || memcmp(again.get(), buf.get(), SRSRAN_CQI_MAX_BITS)) {
          fail("CQI pack -> unpack -> pack", (int)t, combo);
        }
        bool same = true;
        switch (t) {
          case SRSRAN_CQI_TYPE_WIDEBAND:
            same = back.wideband.wideband_cqi == v.wideband.wideband_cqi &&
                   (!c.pmi_present || back.wideband.pmi == v.wideband.pmi) &&
                   (!(c.pmi_present && c.rank_is_not_one) || back.wideband.spatial_diff_cqi == v.wideband.spatial_diff_cqi);
            break;
          case SRSRAN_CQI_TYPE_SUBBAND_UE:
            same = back.subband_ue.subband_cqi == v.subband_ue.subband_cqi &&
                   back.subband_ue.subband_label == v.subband_ue.subband_label;
            break;
          case SRSRAN_CQI_TYPE_SUBBAND_UE_DIFF:
            same = back.subband_ue_diff.wideband_cqi == v.subband_ue_diff.wideband_cqi &&
                   back.subband_ue_diff.subband_diff_cqi == v.subband_ue_diff.subband_diff_cqi;
            break;
          case SRSRAN_CQI_TYPE_SUBBAND_HL:
            same = back.subband_hl.wideband_cqi_cw0 == v.subband_hl.wideband_cqi_cw0 &&
                   back.subband_hl.subband_diff_cqi_cw0 == v.subband_hl.subband_diff_cqi_cw0 &&
                   (!c.rank_is_not_one || (back.subband_hl.wideband_cqi_cw1 == v.subband_hl.wideband_cqi_cw1 &&
                                           back.subband_hl.subband_diff_cqi_cw1 == v.subband_hl.subband_diff_cqi_cw1)) &&
                   (!c.pmi_present || back.subband_hl.pmi == v.subband_hl.pmi);
            break;
        }
        if (!same) {
          fail("CQI round trip changes a field", (int)t, combo);
        }
        printf("cqi %d %u %u %d %d %d %d %d %d %d ", (int)t, c.N, c.L, (int)c.four_antenna_ports, (int)c.pmi_present,
               (int)c.rank_is_not_one, (int)c.subband_label_2_bits, size, n, m);
        print_bits(buf.get(), (uint32_t)n);
        uint32_t w[5];  // the value as the test rebuilds it, by type
        switch (t) {
          case SRSRAN_CQI_TYPE_WIDEBAND:
            w[0] = v.wideband.wideband_cqi, w[1] = v.wideband.spatial_diff_cqi, w[2] = v.wideband.pmi, w[3] = w[4] = 0;
            break;
          case SRSRAN_CQI_TYPE_SUBBAND_UE:
            w[0] = v.subband_ue.subband_cqi, w[1] = v.subband_ue.subband_label, w[2] = w[3] = w[4] = 0;
            break;
          case SRSRAN_CQI_TYPE_SUBBAND_UE_DIFF:
            w[0] = v.subband_ue_diff.wideband_cqi, w[1] = v.subband_ue_diff.subband_diff_cqi, w[2] = w[3] = w[4] = 0;
            break;
          default:
            w[0] = v.subband_hl.wideband_cqi_cw0, w[1] = v.subband_hl.subband_diff_cqi_cw0;
            w[2] = v.subband_hl.wideband_cqi_cw1, w[3] = v.subband_hl.subband_diff_cqi_cw1, w[4] = v.subband_hl.pmi;
        }
        printf(" %u %u %u %u %u\n", w[0], w[1], w[2], w[3], w[4]);
      }
    }
  }
}

void offsets()
{
  for (uint32_t i = 0; i <= 16; i++) {  // 15 and 16 are past the tables: the fallbacks (a message on stderr each)
    const float a = beta_harq(i), r = beta_ri(i), c = beta_cqi(i);
    printf("beta %u %g %g %g %g %g %u %u %u\n", i, srsran_sch_beta_ack(i), srsran_sch_beta_cqi(i), a, r, c,
           srsran_sch_find_Ioffset_ack(a), srsran_sch_find_Ioffset_ri(r), srsran_sch_find_Ioffset_cqi(c));
  }
  for (float b : {10.0f, 1000.0f, 2.0f, 3.0f, 0.5f}) {
    printf("find ack %g %u\nfind ri %g %u\nfind cqi %g %u\n", b, srsran_sch_find_Ioffset_ack(b), b,
           srsran_sch_find_Ioffset_ri(b), b, srsran_sch_find_Ioffset_cqi(b));
  }
}

void coding()
{
  for (uint32_t nin = 1; nin <= 11; nin++) {
    for (uint32_t nout : {32u, 40u}) {
      std::unique_ptr<uint8_t[]> in(new uint8_t[nin]), out(new uint8_t[nout]);
      for (uint32_t i = 0; i < nin; i++) {
        in[i] = (uint8_t)(rnd() & 1);
      }
      memset(out.get(), 0xA5, nout);
      block_encode(in.get(), nin, out.get(), nout);
      printf("block %u %u ", nin, nout);
      print_bits(in.get(), nin);
      putchar(' ');
      print_bits(out.get(), nout);
      putchar('\n');
    }
  }
  for (uint32_t nbits : {12u, 64u}) {
    const uint32_t             Q = 288;  // one PRB, 12 symbols, QPSK: the whole PUSCH of a CQI-only transmission
    std::unique_ptr<uint8_t[]> in(new uint8_t[nbits]), out(new uint8_t[Q]);
    for (uint32_t i = 0; i < nbits; i++) {
      in[i] = (uint8_t)(rnd() & 1);
    }
    memset(out.get(), 0xA5, Q);
    if (!cqi_encode_long(in.get(), nbits, out.get(), Q)) {
      fail("cqi_encode_long", (int)nbits, (int)Q);
    }
    printf("cqilong %u %u ", nbits, Q);
    print_bits(in.get(), nbits);
    putchar(' ');
    print_bits(out.get(), Q);
    putchar('\n');
  }
  std::unique_ptr<uint8_t[]> in(new uint8_t[504]), out(new uint8_t[8]);
  memset(in.get(), 0, 504);
  if (cqi_encode_long(in.get(), 504, out.get(), 8)) {  // SRSRAN_UCI_MAX_CQI_LEN_PUSCH: refused before any access
    fail("cqi_encode_long takes 504 bits", 504, 8);
  }
}

}  // namespace

int main()
{
  segm();
  crc();
  cqi();
  offsets();
  coding();
  if (srsran_mod_bits_x_symbol(SRSRAN_MOD_64QAM) != 6 || srsran_mod_bits_x_symbol((srsran_mod_t)5) != 0) {
    fail("srsran_mod_bits_x_symbol", 0, 0);
  }
  return 0;
}
