// r1d_debug.h -- everything diagnostic builds (make EXTRA=-DGLDM_DEBUG_KNOBS) add to r1d_kernel's launch path (resnet1d.hip):
// the per-wave conv stamps (-DGLDM_WAVE_STAMPS on top), the environment knobs and the stamp report.  In a shipped build the
// macros expand to nothing and the hooks are empty inline functions: the library reads no environment and prints nothing.
// (GLDM_SKIP / GLDM_STAMPS are in r1d_gemm.h.)  resnet1d.hip includes it TWICE inside its
// anonymous namespace: in front of the phase headers for the device part (the stamp macros and arrays), and in front of its
// host side for the hooks, which need what lies between (RunArgs, build_tape, the wave-local chain's g_q_stamp).
//   GLDM_R1D_SKIP=mask       phase-skip mask (GLDM_SKIP)          GLDM_R1D_STAGGER_US=n  start offset of a CU's second workgroup
//   GLDM_R1D_SLOTS=n         persistent workgroups of a launch    GLDM_R1D_ONE_WG=1      one workgroup per CU (LDS request)
//   GLDM_R1D_NOQUAD=1        narrow levels as wide phases         GLDM_R1D_STAMP=1       per-op cycle stamps: blocks, copies, prints

#ifndef GLDM_R1D_DEBUG_DEVICE_PART
#define GLDM_R1D_DEBUG_DEVICE_PART   // ---- first inclusion: the device part

#if defined(GLDM_DEBUG_KNOBS) && defined(GLDM_WAVE_STAMPS)   // per-wave conv stamps cost ~1.5 k cycles per op: their own switch
__device__ long long g_wv_stamp[8][32][8];   // per wave, ring of the last 32 position-major convs: in, k-loop done, out, shape,
                                             // statistics published (in front of the exchange barrier), partners merged
__device__ int g_wv_cnt[8];
#define GLDM_WV_STAMP(c, k, v) \
  do { if (blockIdx.x == 0 && (c).lane == 0) g_wv_stamp[(c).wave][g_wv_cnt[(c).wave] & 31][k] = (v); } while (0)
#define GLDM_WV_NEXT(c) do { if (blockIdx.x == 0 && (c).lane == 0) g_wv_cnt[(c).wave]++; } while (0)
#else
#define GLDM_WV_STAMP(c, k, v) do {} while (0)
#define GLDM_WV_NEXT(c) do {} while (0)
#endif

#elif !defined(GLDM_DEBUG_KNOBS)   // ---- second inclusion: the host hooks; empty in a shipped build

inline int dbg_slots(int slots) { return slots; }
inline size_t dbg_lds_bytes(size_t bytes) { return bytes; }
inline bool dbg_noquad() { return false; }
inline void dbg_arm(RunArgs &) {}
inline void dbg_report(const RunArgs &, bool, bool) {}

#else

// co-residence experiment: fewer persistent workgroups than CUs, so that another stream's kernels find free
// CUs while the fused launch runs
inline int dbg_slots(int slots) {
  const char *e = getenv("GLDM_R1D_SLOTS");
  return e && atoi(e) > 0 ? atoi(e) : slots;
}
inline size_t dbg_lds_bytes(size_t bytes) {   // one workgroup per CU: phases on their own
  return getenv("GLDM_R1D_ONE_WG") && bytes < 100 * 1024 ? 100 * 1024 : bytes;
}
inline bool dbg_noquad() { return getenv("GLDM_R1D_NOQUAD") != nullptr; }   // A/B: the narrow levels as position-major phases

// Phase skipping, the start offset of the second workgroup of a CU, and the device buffer of the per-op cycle stamps
// (kMaxOps + 2 of them: one per op, the end of the last op, the start of the step prologue)
inline void dbg_arm(RunArgs &a) {
  const char *e = getenv("GLDM_R1D_SKIP");
  a.skip = e ? atoi(e) : 0;
  const char *g = getenv("GLDM_R1D_STAGGER_US");
  a.stagger_ticks = g ? atoi(g) * 100 : 0;
  static long long *dstamps = nullptr;
  const bool stamp = getenv("GLDM_R1D_STAMP") != nullptr;
  if (stamp && !dstamps) (void)hipMalloc(&dstamps, (kMaxOps + 2) * sizeof(long long));
  a.stamps = stamp ? dstamps : nullptr;
}

// The stamp report of the launch just made (GLDM_R1D_STAMP): waits for it, copies the stamps of workgroup 0's last step and
// prints one line per op, labelled from the tape the launch ran (the 32-column engine builds the same tape in the kernel),
// then the wave-local chain's stages per quad and, with GLDM_WAVE_STAMPS, the last 32 wide convs per wave.
inline void dbg_report(const RunArgs &a, bool pm, bool pm16) {
  if (!a.stamps) return;
  static long long host[kMaxOps + 2];
  static int own_tape[kMaxOps * kOpInts];
  static const char *names[] = {"", "CONV", "RES4", "LN", "ATT", "QKVLN", "OUTLN", "QKVAT", "QUAD"};
  (void)hipDeviceSynchronize();
  (void)hipMemcpy(host, a.stamps, sizeof(host), hipMemcpyDeviceToHost);
  const int *tape = pm ? a.pm_tape : own_tape;
  const int n_ops = pm ? a.pm_nops : build_tape<kEngineNC>(a.d, own_tape);
  const bool quad = n_ops > 0 && tape[0] == OP_QUAD;
  for (int op = 0; op < n_ops; ++op) {
    const int *o = tape + kOpInts * op;
    int C = 0, cout = 0, taps = 0;   // r1d_tape.h: the op layout
    switch (o[0]) {
      case OP_CONV: C = o[5]; cout = o[6]; taps = o[7] & 255; break;
      case OP_RES4: C = cout = 4; taps = 3; break;             // the 4-channel level's ResnetBlock
      case OP_LN: C = cout = o[4]; break;
      case OP_ATT: C = (o - kOpInts)[5]; cout = 64; break;     // one head pair of the qkv conv in front of it
      case OP_QKVATT: C = o[4]; cout = 384; taps = 1; break;
      case OP_OUTLN: C = o[5]; cout = o[6]; taps = 1; break;
      case OP_QUAD: C = a.d.dims[0]; cout = 128; taps = 3; break;   // the levels in front of the 128-channel one
    }
    printf("op %3d %-5s C=%3d cout=%3d k=%d : %7lld clk\n", op, names[o[0]], C, cout, taps, host[op + 1] - host[op]);
  }
  printf("step total (ops): %lld clk; step prologue (embedding sums, init conv): %lld clk\n", host[n_ops] - host[0],
         host[0] - host[kMaxOps + 1]);
  if (quad) {
    static long long qs[4][16];
    (void)hipMemcpyFromSymbol(qs, HIP_SYMBOL(g_q_stamp), sizeof(qs));   // quad_narrow.h
    static const char *qn4[] = {"pads", "rb4", "rb4", "att4", "down4", "rb32", "rb32", "att32", "down32", "rb64", "rb64", "att64", "down64"};
    static const char *qn16[] = {"pads", "rb16", "rb16", "att16", "down16", "rb32", "rb32", "att32", "down32", "rb64", "rb64", "att64", "down64"};
    const char **qn = pm16 ? qn16 : qn4;
    for (int q = 0; q < 4; ++q) {
      printf("quad %d:", q);
      for (int i = 1; i <= 12; ++i) printf(" %s %lld", qn[i], qs[q][i] - qs[q][i - 1]);
      printf(" | total %lld, polls that waited %lld\n", qs[q][12] - qs[q][0], qs[q][13]);
    }
  }
#ifdef GLDM_WAVE_STAMPS
  if (pm) {   // per-wave view of the last 32 position-major convs of workgroup 0: k-loop / epilogue, relative to wave 0's entry
    static long long wv[8][32][8];
    int cnt[8];
    (void)hipMemcpyFromSymbol(wv, HIP_SYMBOL(g_wv_stamp), sizeof(wv));
    (void)hipMemcpyFromSymbol(cnt, HIP_SYMBOL(g_wv_cnt), sizeof(cnt));
    for (int i = 0; i < 32; ++i) {
      const int e = (cnt[0] + i) & 31;
      printf("conv %3lld->%3lld:", wv[0][e][3] / 1000, wv[0][e][3] % 1000);
      for (int w = 0; w < 8; ++w)
        printf("  w%d in %+5lld loop %6lld epi %6lld (stats %5lld wait %5lld finish %5lld) |", w, wv[w][e][0] - wv[0][e][0],
               wv[w][e][1] - wv[w][e][0], wv[w][e][2] - wv[w][e][1], wv[w][e][4] - wv[w][e][1], wv[w][e][5] - wv[w][e][4],
               wv[w][e][2] - wv[w][e][5]);
      printf("\n");
    }
  }
#endif
}

#endif
