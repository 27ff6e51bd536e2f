// TEST INFRASTRUCTURE ONLY: dcn_pick of csrc/dcn_fused.hip (which instantiation a grouped DCNv2 launch runs) against the table it was
// written from -- the choice the dispatcher made when choosing and launching were one function, transcribed by hand, never computed by
// calling dcn_pick.  Includes the emulation's copy of the source (tests/simt/_build/src) and links the emulation library; built once as it
// is (the 16-bit builds' table) and once with -DMQ_F32 (the split-precise build's).  tests/test_simt_kernels_cpu.py compiles and runs it.
#include "dcn_fused.cpp"
#include <stdio.h>

MQ_NAMESPACE_BEGIN
struct PickRow { int nw, sync; bool p, tiled; int want_nw, want_sync; bool want_plain, want_bdma; };   // p = plain && plain_on
static const PickRow PICK_TABLE[16] = {
#if !defined(MQ_F32)
    // tiled weights: (nw, 1, P, true)
    {8, 1, false, true, 8, 1, false, true},     {8, 1, true, true, 8, 1, true, true},
    {8, 2, false, true, 8, 1, false, true},     {8, 2, true, true, 8, 1, true, true},
    {16, 1, false, true, 16, 1, false, true},   {16, 1, true, true, 16, 1, true, true},
    {16, 2, false, true, 16, 1, false, true},   {16, 2, true, true, 16, 1, true, true},
    // row-major weights: 16 waves, one barrier: (16, 1, P, false); two: (16, 2, false, false); 8 waves: (8, 2, false, false)
    {16, 1, false, false, 16, 1, false, false}, {16, 1, true, false, 16, 1, true, false},
    {16, 2, false, false, 16, 2, false, false}, {16, 2, true, false, 16, 2, false, false},
    {8, 1, false, false, 8, 2, false, false},   {8, 1, true, false, 8, 2, false, false},
    {8, 2, false, false, 8, 2, false, false},   {8, 2, true, false, 8, 2, false, false},
#else
    // tiled weights: (8, 1, P, true) whatever nw and sync
    {8, 1, false, true, 8, 1, false, true},     {8, 1, true, true, 8, 1, true, true},
    {8, 2, false, true, 8, 1, false, true},     {8, 2, true, true, 8, 1, true, true},
    {16, 1, false, true, 8, 1, false, true},    {16, 1, true, true, 8, 1, true, true},
    {16, 2, false, true, 8, 1, false, true},    {16, 2, true, true, 8, 1, true, true},
    // row-major weights, 8 waves: P ? (8, 1, true, false) : (8, sync, false, false); 16 waves: as the 16-bit builds
    {8, 1, false, false, 8, 1, false, false},   {8, 1, true, false, 8, 1, true, false},
    {8, 2, false, false, 8, 2, false, false},   {8, 2, true, false, 8, 1, true, false},
    {16, 1, false, false, 16, 1, false, false}, {16, 1, true, false, 16, 1, true, false},
    {16, 2, false, false, 16, 2, false, false}, {16, 2, true, false, 16, 2, false, false},
#endif
};

static int dcn_pick_check() {
  int bad = 0, seen = 0;
  for (int nw = 8; nw <= 16; nw += 8)
    for (int sync = 1; sync <= 2; ++sync)
      for (int plain = 0; plain < 2; ++plain)
        for (int plain_on = 0; plain_on < 2; ++plain_on)
          for (int tiled = 0; tiled < 2; ++tiled) {
            const bool p = plain && plain_on;
            const PickRow* row = nullptr;
            for (const PickRow& r : PICK_TABLE)
              if (r.nw == nw && r.sync == sync && r.p == p && r.tiled == (bool)tiled) row = &r;
            if (!row) { ++bad; printf("no row for nw %d sync %d p %d tiled %d\n", nw, sync, (int)p, tiled); continue; }
            ++seen;
            const DcnPick k = dcn_pick(nw, sync, p, (bool)tiled);
            if (k.nw != row->want_nw || k.sync != row->want_sync || k.plain != row->want_plain || k.bdma != row->want_bdma) {
              ++bad;
              printf("nw %d sync %d plain %d plain_on %d tiled %d: (%d, %d, %d, %d), expected (%d, %d, %d, %d)\n", nw, sync, plain, plain_on, tiled,
                     k.nw, k.sync, (int)k.plain, (int)k.bdma, row->want_nw, row->want_sync, (int)row->want_plain, (int)row->want_bdma);
            }
          }
  if (seen != 32) { ++bad; printf("%d combinations, expected 32\n", seen); }
  return bad;
}
MQ_NAMESPACE_END

#if defined(MQ_F32)
using namespace mq_f32;
#endif
int main() {
  const int bad = dcn_pick_check();
  printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
