// r1d_tape.h -- the step program of r1d_kernel (resnet1d.hip): op codes, the 12-int op layout, which descriptors run their
// narrow levels wave-local (quad_levels, quad16_levels), build_tape (host: the 64-column engines, the tape travels in the
// kernel arguments; device: the 32-column engine, into LDS) and read_op.  Included by resnet1d.hip inside its anonymous
// namespace, in front of the phase headers.

// One denoiser / decoder step is a fixed program of barrier-separated ops (45 for the shipped
// denoiser: per level 2 x [conv+GN, conv+GN+residual], LN, 2 x [qkv conv, attention], out conv, LN,
// down conv).  It is written once per workgroup into LDS (12 ints per op) and interpreted by a switch
// inside the step loop, so every phase body exists once, inlined, with registers allocated across the
// whole kernel: no calls, no callee-save traffic and no spilled kernel state between phases.
enum { OP_CONV = 1, OP_RES4 = 2, OP_LN = 3, OP_ATT = 4, OP_QKVLN = 5, OP_OUTLN = 6, OP_QKVATT = 7, OP_QUAD = 8 };
// An op is kOpInts = 12 ints, o[0] its code; weight / bias / gain entries are float offsets into the packed weights, src / dst
// float offsets into LDS (R1dGeo<NC>::kBuf*):
//   OP_CONV    w, bias, src, dst, cin, cout, flags, GroupNorm gamma, beta, scale/shift W, scale/shift b
//              flags (int 7): taps | alias << 8 | GroupNorm epilogue mode << 9 | fused << 11 | (scale/shift table offset / 4) << 12
//   OP_RES4    conv1 w, b, norm1 gamma, beta, conv2 w, b, norm2 gamma, beta, scale/shift W, b, barrier behind the op
//   OP_LN      src, dst (-1: none), residual (-1: none), C, gain
//   OP_ATT     qkv, out
//   OP_QKVATT  w (PreNorm gain folded in), s = W' 1, src, C
//   OP_OUTLN   w, bias, src, residual stream, cin, C, gain
//   OP_QUAD    (none: the wave-local narrow levels read the descriptor)
// (OP_QKVLN is not emitted any more.)  The stamp report of diagnostic builds (r1d_debug.h) labels its lines from these ints.
constexpr int kOpInts = 12, kMaxOps = 84;  // op tape: 84 * 12 = 1008 ints; the op count lives in int 1023
constexpr int kPmMaxOps = 8 * GLDM_R1D_MAX_LEVELS + 2;   // 64-column engines: at most 8 entries per level + the last ResnetBlock's 2
// The levels of 4, 32 and 64 channels in front of a 128-channel one run wave-local (quad_narrow.h): the shipped denoiser
__host__ __device__ __forceinline__ bool quad_levels(const gldm_r1d_desc &d) {
  return d.seq_len == 4 && d.emb_dim == 16 && d.n_levels >= 3 && d.dims[0] == 4 && d.dims[1] == 32 && d.dims[2] == 64 &&
         d.dims[3] == 128 && d.lv[0].out_wq > 0 && d.lv[1].out_wq > 0 && d.lv[1].qkvn_wq > 0 && d.lv[1].down_wq > 0 &&
         d.lv[2].out_wq > 0 && d.lv[2].qkvn_wq > 0 && d.lv[2].down_wq > 0 && d.rb[2].c1_wq > 0 && d.rb[2].c2_wq > 0 &&
         d.rb[3].c1_wq > 0 && d.rb[3].c2_wq > 0 && d.rb[4].c1_wq > 0 && d.rb[4].c2_wq > 0 && d.rb[5].c1_wq > 0 && d.rb[5].c2_wq > 0;
}
// The same for the 16-position nets (quad16_narrow.h): levels of 16, 32 and 64 channels in front of a 128-channel one.  The
// scale / shift rows come from the per-cloud table (pose decoder: ss_table_rows) or the 64-wide embedding (the launcher
// checks that one of the two holds).
__host__ __device__ __forceinline__ bool quad16_levels(const gldm_r1d_desc &d) {
  return d.seq_len == 16 && d.groups == 4 && d.n_levels >= 3 && d.dims[0] == 16 && d.dims[1] == 32 && d.dims[2] == 64 && d.dims[3] == 128 &&
         d.lv[0].out_wq > 0 && d.lv[0].qkvn_wq > 0 && d.lv[0].down_wq > 0 && d.lv[1].out_wq > 0 && d.lv[1].qkvn_wq > 0 &&
         d.lv[1].down_wq > 0 && d.lv[2].out_wq > 0 && d.lv[2].qkvn_wq > 0 && d.lv[2].down_wq > 0 && d.rb[0].c1_wq > 0 &&
         d.rb[0].c2_wq > 0 && d.rb[1].c1_wq > 0 && d.rb[1].c2_wq > 0 && d.rb[2].c1_wq > 0 && d.rb[2].c2_wq > 0 && d.rb[3].c1_wq > 0 &&
         d.rb[3].c2_wq > 0 && d.rb[4].c1_wq > 0 && d.rb[4].c2_wq > 0 && d.rb[5].c1_wq > 0 && d.rb[5].c2_wq > 0;
}
// conv flags (int 7 of OP_CONV, above)
constexpr int kFlagAlias = 1 << 8;
constexpr int kFlagFused = 1 << 11;   // position-major engine: this conv and the next tape entry are one ResnetBlock op
constexpr int kFlagTabShift = 12;

// GroupNorm rides in the conv epilogue: the rows of a group must sit inside one wave's accumulators
__host__ __device__ __forceinline__ bool gn_fusable(int C, int groups) {
  if (groups != 4 || C % 4) return false;
  const int cpg = C / 4;
  return cpg == 1 || cpg == 4 || cpg == 8 || (cpg % 16 == 0 && cpg <= 64);
}

template <int NC>
__host__ __device__ __forceinline__ int build_tape(const gldm_r1d_desc &d, int *tape, bool use_quad = true) {
  using GG = R1dGeo<NC>;
  int n = 0;
  auto emit = [&](int type, int a1 = 0, int a2 = 0, int a3 = 0, int a4 = 0, int a5 = 0, int a6 = 0, int a7 = 0,
                  int a8 = 0, int a9 = 0, int a10 = 0, int a11 = 0) {
    int *o = tape + kOpInts * n++;
    o[0] = type; o[1] = a1; o[2] = a2; o[3] = a3; o[4] = a4; o[5] = a5; o[6] = a6; o[7] = a7;
    o[8] = a8; o[9] = a9; o[10] = a10; o[11] = a11;
  };
  constexpr int X = GG::kBufX, H = GG::kBufH, Y = GG::kBufY, O = GG::kBufO, QKV = GG::kBufQKV;
  int tab_off = 0;  // rows [2C] of every ResnetBlock, in block order (ss_table_kernel writes the same layout)
  auto resblock = [&](const gldm_r1d_resblock &rb, int C, bool last_of_pair) {
    const int toff = tab_off;
    tab_off += 2 * C;
    if (C == 4 && d.seq_len == 4) {  // one-wave VALU form; the barrier comes after the second block
      emit(OP_RES4, rb.c1_w, rb.c1_b, rb.n1_w, rb.n1_b, rb.c2_w, rb.c2_b, rb.n2_w, rb.n2_b, rb.ss_w, rb.ss_b,
           last_of_pair ? 1 : 0);
      return;
    }
    // the position-major engine reads the split-f16 copies of the conv weights (gemm_pm3_bf)
    emit(OP_CONV, NC == 64 ? rb.c1_w3 : rb.c1_w, rb.c1_b, X, H, C, C,
         3 | (1 << 9) | (NC == 64 ? kFlagFused : 0) | ((toff >> 2) << kFlagTabShift), rb.n1_w, rb.n1_b, rb.ss_w, rb.ss_b);
    emit(OP_CONV, NC == 64 ? rb.c2_w3 : rb.c2_w, rb.c2_b, H, X, C, C, 3 | (2 << 9), rb.n2_w, rb.n2_b, -1, 0);  // X += act(GN(conv(H)))
  };
  const bool quad = NC == 64 && use_quad && (quad_levels(d) || quad16_levels(d));
  if (quad) emit(OP_QUAD);
  // constant indices only: a dynamically indexed kernel argument is copied to scratch memory
#pragma unroll
  for (int lv = 0; lv < GLDM_R1D_MAX_LEVELS; ++lv) {
    if (quad && lv < 3) { tab_off += 4 * d.dims[lv]; continue; }   // two ResnetBlocks' table rows each (16-position engine only)
    if (lv < d.n_levels) {
      const int C = d.dims[lv], Cn = d.dims[lv + 1];
      resblock(d.rb[2 * lv], C, false);
      resblock(d.rb[2 * lv + 1], C, true);
      const gldm_r1d_level &v = d.lv[lv];
      // position-major engine (C <= 128 at attention levels): X rows [0, 128) | q,k,v of the four heads: 384 rows, o in
      // place of q.  The PreNorm LayerNorm is folded into the qkv conv (C = 4: computed in the lanes of the qkv phase).
      int Oa = O;
      if (NC == 64) {   // PreNorm + to_qkv + attention core of the four heads: one op, the output as planes (kPlaneH)
        emit(OP_QKVATT, C == 4 ? v.qkvn_w : v.qkvn_w3, v.qkvn_s, X, C);
        Oa = PG<4>::kH;   // (kPlaneH of r1d_wide.h)
      } else {
        emit(OP_LN, X, Y, -1, C, v.ln_g);
        emit(OP_CONV, v.qkv_w[0], -1, Y, QKV, C, 192, 1);
        emit(OP_ATT, QKV, O);
        emit(OP_CONV, v.qkv_w[1], -1, Y, QKV, C, 192, 1);
        emit(OP_ATT, QKV, O + 64 * NC);
      }
      if (NC == 64 && (C == 4 || C == 16 || C == 32 || C == 64 || C == 128)) {  // to_out conv + LayerNorm + residual: one phase
        emit(OP_OUTLN, v.out_w3, v.out_b, Oa, X, kHidden, C, v.ln2_g);
      } else {
        emit(OP_CONV, v.out_w, v.out_b, Oa, Y, kHidden, C, 1);
        emit(OP_LN, Y, -1, X, C, v.ln2_g);
      }
      emit(OP_CONV, (NC == 64 && C >= 16) ? v.down_w3 : v.down_w, v.down_b, X, X, C, Cn, 3 | kFlagAlias);
    }
  }
#pragma unroll
  for (int lv = 1; lv <= GLDM_R1D_MAX_LEVELS; ++lv)
    if (lv == d.n_levels) resblock(d.rb[2 * lv], d.dims[lv], true);
  return n;
}

// One tape entry -> 12 wave-uniform ints.  LDS tape (sample-major engines): three 16-byte reads + v_readfirstlane;
// kernarg tape (position-major engine): scalar loads from the constant address space, no vector instruction at all.
typedef __attribute__((address_space(4))) const int kernarg_int;
typedef __attribute__((ext_vector_type(4))) int i32x4;
template <bool KARG>
__device__ __forceinline__ void read_op(const int *tape, kernarg_int *ktape, int op, int (&o)[kOpInts]) {
  if constexpr (KARG) {
    typedef __attribute__((address_space(4))) const i32x4 kernarg_i4;
    kernarg_i4 *t4 = reinterpret_cast<kernarg_i4 *>(ktape + kOpInts * op);
    const i32x4 q0 = t4[0], q1 = t4[1], q2 = t4[2];
    o[0] = q0.x; o[1] = q0.y; o[2] = q0.z; o[3] = q0.w; o[4] = q1.x; o[5] = q1.y; o[6] = q1.z; o[7] = q1.w;
    o[8] = q2.x; o[9] = q2.y; o[10] = q2.z; o[11] = q2.w;
  } else {
    const int4 *t4 = reinterpret_cast<const int4 *>(tape + kOpInts * op);
    const int4 q0 = t4[0], q1 = t4[1], q2 = t4[2];
    o[0] = q0.x; o[1] = q0.y; o[2] = q0.z; o[3] = q0.w; o[4] = q1.x; o[5] = q1.y; o[6] = q1.z; o[7] = q1.w;
    o[8] = q2.x; o[9] = q2.y; o[10] = q2.z; o[11] = q2.w;
#pragma unroll
    for (int i = 0; i < kOpInts; ++i) o[i] = __builtin_amdgcn_readfirstlane(o[i]);
  }
}
