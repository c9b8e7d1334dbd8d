// Issue cost of the integer VALU instructions of the ChaCha20 and Poly1305
// inner loops on gfx950: cycles per wave-instruction per SIMD with 1 and 4
// waves per SIMD, 8 independent chains per wave (s_memtime around a fixed
// unrolled stream).  Build: hipcc --offload-arch=gfx950 -O3 -o valu_rate valu_rate.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
  printf("%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); return 1; } } while (0)

constexpr int kIters = 256;

#define BODY8(INSN)                                                   \
  asm volatile(INSN(0) INSN(1) INSN(2) INSN(3) INSN(4) INSN(5) INSN(6) INSN(7) \
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), \
                 "+v"(r[6]), "+v"(r[7]) : "v"(a), "v"(b) : "s40", "s41");

// The same with an SGPR operand (%10), as the GCM rounds hold their masks.
#define BODY8S(INSN)                                                  \
  asm volatile(INSN(0) INSN(1) INSN(2) INSN(3) INSN(4) INSN(5) INSN(6) INSN(7) \
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), \
                 "+v"(r[6]), "+v"(r[7]) : "v"(a), "v"(b), "s"(sm));

// 64-bit register pairs for the mad/shift cases.
#define BODY8_64(INSN)                                                  \
  asm volatile(INSN(0) INSN(1) INSN(2) INSN(3) INSN(4) INSN(5) INSN(6) INSN(7) \
               : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), \
                 "+v"(w[6]), "+v"(w[7]) : "v"(a), "v"(b) : "s40", "s41");

#define I_ADD(i) "v_add_u32 %" #i ", %" #i ", %8\n"
#define I_XOR(i) "v_xor_b32 %" #i ", %" #i ", %8\n"
#define I_ALIGNBIT(i) "v_alignbit_b32 %" #i ", %" #i ", %" #i ", 16\n"
#define I_BITOP3(i) "v_bitop3_b32 %" #i ", %" #i ", %8, %9 bitop3:0x96\n"
#define I_MULLO(i) "v_mul_lo_u32 %" #i ", %" #i ", %8\n"
#define I_MULHI(i) "v_mul_hi_u32 %" #i ", %" #i ", %8\n"
#define I_MAD64(i) "v_mad_u64_u32 %" #i ", s[40:41], %8, %9, %" #i "\n"
#define I_SHR64(i) "v_lshrrev_b64 %" #i ", 26, %" #i "\n"
#define I_ADD64(i) "v_lshl_add_u64 %" #i ", %" #i ", 0, %" #i "\n"
#define I_PERM(i) "v_perm_b32 %" #i ", %" #i ", %" #i ", %9\n"
#define I_ALIGNBYTE(i) "v_alignbyte_b32 %" #i ", %" #i ", %" #i ", 2\n"
#define I_LSHLOR(i) "v_lshl_or_b32 %" #i ", %" #i ", 7, %8\n"
#define I_XAD(i) "v_xad_u32 %" #i ", %" #i ", %8, %9\n"
#define I_ADD3(i) "v_add3_u32 %" #i ", %" #i ", %8, %9\n"
#define I_LSHL(i) "v_lshlrev_b32 %" #i ", 7, %" #i "\n"
#define I_XOR_SDWA(i) "v_xor_b32_sdwa %" #i ", %" #i ", %8 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_0 src1_sel:WORD_0\n"
#define I_PK_ADD16(i) "v_pk_add_u16 %" #i ", %" #i ", %8 op_sel:[1,1] op_sel_hi:[0,0]\n"

// Address forms of the GCM T-table lookups (a state byte into bits 8..15 over
// a lane constant): bitop3 with its mask in an SGPR, SDWA byte moves into
// byte 1 of a register that keeps its other bytes (chain through the
// preserved destination), and the three-operand mask/insert/extract ops.
#define I_BITOP3_S(i) "v_bitop3_b32 %" #i ", %" #i ", %10, %9 bitop3:0xea\n"
// (which of the two makes the case above slow: the SGPR or the truth table;
// and whether an SGPR source slows a VOP2 op as well)
#define I_BITOP3_S96(i) "v_bitop3_b32 %" #i ", %" #i ", %8, %10 bitop3:0x96\n"
#define I_BITOP3_VSEL(i) "v_bitop3_b32 %" #i ", %" #i ", %8, %9 bitop3:0xdc\n"
#define I_XOR_S(i) "v_xor_b32 %" #i ", %10, %" #i "\n"
#define I_MOV_SDWA0(i) "v_mov_b32_sdwa %" #i ", %8 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_0\n"
#define I_MOV_SDWA2(i) "v_mov_b32_sdwa %" #i ", %8 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_2\n"
#define I_MOV_SDWA3(i) "v_mov_b32_sdwa %" #i ", %8 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_3\n"
// (as the rounds would use it: one register rewritten by every instruction,
// each from another source register)
#define I_MOV_SDWA_ONE(i) "v_mov_b32_sdwa %0, %" #i " dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_2\n"
#define I_OR_SDWA(i) "v_or_b32_sdwa %" #i ", %" #i ", %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD\n"
#define I_BFI(i) "v_bfi_b32 %" #i ", %9, %" #i ", %8\n"
#define I_AND_OR(i) "v_and_or_b32 %" #i ", %" #i ", %9, %8\n"
#define I_BFE(i) "v_bfe_u32 %" #i ", %" #i ", 8, 8\n"
// v_readlane_b32 writes an SGPR: eight destinations (s40..s47), sources the
// eight chain registers; nothing reads the results inside the stream.
#define I_READLANE(i) "v_readlane_b32 s4" #i ", %" #i ", 3\n"
#define BODY8_RL asm volatile(I_READLANE(0) I_READLANE(1) I_READLANE(2) I_READLANE(3) I_READLANE(4) I_READLANE(5) I_READLANE(6) I_READLANE(7) \
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), \
                 "+v"(r[6]), "+v"(r[7]) : "v"(a), "v"(b) : "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47");

// ChaCha quarter-round-like dependent triples (add, xor, rotate) on ILP
// independent chains.
#define QSTEP(i) "v_add_u32 %" #i ", %" #i ", %8\n v_xor_b32 %" #i ", %" #i ", %9\n v_alignbit_b32 %" #i ", %" #i ", %" #i ", 16\n"
#define QBODY4 asm volatile(QSTEP(0) QSTEP(1) QSTEP(2) QSTEP(3) : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]) : "v"(a), "v"(b));
#define QBODY8 asm volatile(QSTEP(0) QSTEP(1) QSTEP(2) QSTEP(3) QSTEP(4) QSTEP(5) QSTEP(6) QSTEP(7) : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]) : "v"(a), "v"(b));

template <int K>
__global__ void rate(uint64_t *out, uint32_t a, uint32_t b) {
  const uint32_t sm = __builtin_amdgcn_readfirstlane(b) | 0xff00u;  // an SGPR operand
  uint32_t r[8];
  uint64_t w[8];
  for (int i = 0; i < 8; i++) { r[i] = threadIdx.x + i; w[i] = threadIdx.x * 3ull + i; }
  if (K == 16) for (int i = 0; i < 8; i++) r[i] = 0;
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < kIters; it++) {
    if (K == 0) { BODY8(I_ADD) BODY8(I_ADD) BODY8(I_ADD) BODY8(I_ADD) }
    if (K == 1) { BODY8(I_XOR) BODY8(I_XOR) BODY8(I_XOR) BODY8(I_XOR) }
    if (K == 2) { BODY8(I_ALIGNBIT) BODY8(I_ALIGNBIT) BODY8(I_ALIGNBIT) BODY8(I_ALIGNBIT) }
    if (K == 3) { BODY8(I_BITOP3) BODY8(I_BITOP3) BODY8(I_BITOP3) BODY8(I_BITOP3) }
    if (K == 4) { BODY8(I_MULLO) BODY8(I_MULLO) BODY8(I_MULLO) BODY8(I_MULLO) }
    if (K == 5) { BODY8(I_MULHI) BODY8(I_MULHI) BODY8(I_MULHI) BODY8(I_MULHI) }
    if (K == 6) { BODY8_64(I_MAD64) BODY8_64(I_MAD64) BODY8_64(I_MAD64) BODY8_64(I_MAD64) }
    if (K == 7) { BODY8_64(I_SHR64) BODY8_64(I_SHR64) BODY8_64(I_SHR64) BODY8_64(I_SHR64) }
    if (K == 8) { BODY8_64(I_ADD64) BODY8_64(I_ADD64) BODY8_64(I_ADD64) BODY8_64(I_ADD64) }
    if (K == 9) { BODY8(I_PERM) BODY8(I_PERM) BODY8(I_PERM) BODY8(I_PERM) }
    if (K == 10) { BODY8(I_ALIGNBYTE) BODY8(I_ALIGNBYTE) BODY8(I_ALIGNBYTE) BODY8(I_ALIGNBYTE) }
    if (K == 11) { BODY8(I_LSHLOR) BODY8(I_LSHLOR) BODY8(I_LSHLOR) BODY8(I_LSHLOR) }
    if (K == 12) { BODY8(I_XAD) BODY8(I_XAD) BODY8(I_XAD) BODY8(I_XAD) }
    if (K == 13) { BODY8(I_ADD3) BODY8(I_ADD3) BODY8(I_ADD3) BODY8(I_ADD3) }
    if (K == 14) { BODY8(I_LSHL) BODY8(I_LSHL) BODY8(I_LSHL) BODY8(I_LSHL) }
    // power probes: same instruction, operands that toggle all bits / none
    if (K == 15) { BODY8(I_XOR) BODY8(I_XOR) BODY8(I_XOR) BODY8(I_XOR) }
    if (K == 16) { BODY8(I_ALIGNBIT) BODY8(I_ALIGNBIT) BODY8(I_ALIGNBIT) BODY8(I_ALIGNBIT) }
    // 32 instructions per iteration in both: ILP 4 (the QR interleave of one
    // ChaCha block) vs ILP 8 (two blocks interleaved); order within a step
    // keeps each chain's add -> xor -> rotate dependent.
    if (K == 17) { QBODY4 QBODY4 asm volatile("v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n" : "+v"(r[5]) : "v"(a)); }
    if (K == 19) { BODY8(I_XOR_SDWA) BODY8(I_XOR_SDWA) BODY8(I_XOR_SDWA) BODY8(I_XOR_SDWA) }
    if (K == 20) { BODY8(I_PK_ADD16) BODY8(I_PK_ADD16) BODY8(I_PK_ADD16) BODY8(I_PK_ADD16) }
    if (K == 21) { BODY8S(I_BITOP3_S) BODY8S(I_BITOP3_S) BODY8S(I_BITOP3_S) BODY8S(I_BITOP3_S) }
    if (K == 22) { BODY8(I_MOV_SDWA0) BODY8(I_MOV_SDWA0) BODY8(I_MOV_SDWA0) BODY8(I_MOV_SDWA0) }
    if (K == 23) { BODY8(I_MOV_SDWA2) BODY8(I_MOV_SDWA2) BODY8(I_MOV_SDWA2) BODY8(I_MOV_SDWA2) }
    if (K == 24) { BODY8(I_MOV_SDWA3) BODY8(I_MOV_SDWA3) BODY8(I_MOV_SDWA3) BODY8(I_MOV_SDWA3) }
    if (K == 25) { BODY8(I_MOV_SDWA_ONE) BODY8(I_MOV_SDWA_ONE) BODY8(I_MOV_SDWA_ONE) BODY8(I_MOV_SDWA_ONE) }
    if (K == 26) { BODY8(I_OR_SDWA) BODY8(I_OR_SDWA) BODY8(I_OR_SDWA) BODY8(I_OR_SDWA) }
    if (K == 27) { BODY8(I_BFI) BODY8(I_BFI) BODY8(I_BFI) BODY8(I_BFI) }
    if (K == 28) { BODY8(I_AND_OR) BODY8(I_AND_OR) BODY8(I_AND_OR) BODY8(I_AND_OR) }
    if (K == 29) { BODY8(I_BFE) BODY8(I_BFE) BODY8(I_BFE) BODY8(I_BFE) }
    if (K == 30) { BODY8_RL BODY8_RL BODY8_RL BODY8_RL }
    if (K == 31) { BODY8S(I_BITOP3_S96) BODY8S(I_BITOP3_S96) BODY8S(I_BITOP3_S96) BODY8S(I_BITOP3_S96) }
    if (K == 32) { BODY8(I_BITOP3_VSEL) BODY8(I_BITOP3_VSEL) BODY8(I_BITOP3_VSEL) BODY8(I_BITOP3_VSEL) }
    if (K == 33) { BODY8S(I_XOR_S) BODY8S(I_XOR_S) BODY8S(I_XOR_S) BODY8S(I_XOR_S) }
    if (K == 18) { QBODY8 asm volatile("v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n v_add_u32 %0, %0, %1\n" : "+v"(r[5]) : "v"(a)); }
  }
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  uint64_t acc = 0;
  for (int i = 0; i < 8; i++) acc += r[i] + w[i];
  if ((threadIdx.x & 63) == 0) out[blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64] = t1 - t0;
  if (acc == 0x123456789ull) out[0] = acc;
}

int main() {
  const char *names[] = {"v_add_u32", "v_xor_b32", "v_alignbit_b32", "v_bitop3_b32", "v_mul_lo_u32",
                         "v_mul_hi_u32", "v_mad_u64_u32", "v_lshrrev_b64", "v_lshl_add_u64",
                         "v_perm_b32", "v_alignbyte_b32", "v_lshl_or_b32", "v_xad_u32", "v_add3_u32",
                         "v_lshlrev_b32", "v_xor_b32 ~0", "v_alignbit(0)", "QR ILP4(+8 add)", "QR ILP8(+8 add)",
                         "v_xor_b32_sdwa", "v_pk_add_u16", "v_bitop3 (SGPR)", "v_mov_sdwa B0>B1",
                         "v_mov_sdwa B2>B1", "v_mov_sdwa B3>B1", "v_mov_sdwa 1dst", "v_or_b32_sdwa",
                         "v_bfi_b32", "v_and_or_b32", "v_bfe_u32", "v_readlane_b32",
                         "v_bitop3 SGPR 96", "v_bitop3 VGPR dc", "v_xor_b32 (SGPR)"};
  uint64_t *d;
  CK(hipMalloc(&d, 1 << 20));
  uint64_t h[4096];
  // s_memtime counts shader-clock cycles; the ratio to v_add_u32 under the
  // same occupancy is reported beside them.
  for (int waves = 1; waves <= 4; waves *= 4) {
    double base = 0;
    for (int k = 0; k < 34; k++) {
      for (int rep = 0; rep < 2; rep++) {
        // one workgroup per CU, `waves` waves per SIMD
        const int threads = 256 * waves;
        switch (k) {
          case 0: rate<0><<<256, threads>>>(d, 3, 5); break;
          case 1: rate<1><<<256, threads>>>(d, 3, 5); break;
          case 2: rate<2><<<256, threads>>>(d, 3, 5); break;
          case 3: rate<3><<<256, threads>>>(d, 3, 5); break;
          case 4: rate<4><<<256, threads>>>(d, 3, 5); break;
          case 5: rate<5><<<256, threads>>>(d, 3, 5); break;
          case 6: rate<6><<<256, threads>>>(d, 3, 5); break;
          case 7: rate<7><<<256, threads>>>(d, 3, 5); break;
          case 8: rate<8><<<256, threads>>>(d, 3, 5); break;
          case 9: rate<9><<<256, threads>>>(d, 3, 0x05040706); break;
          case 10: rate<10><<<256, threads>>>(d, 3, 5); break;
          case 11: rate<11><<<256, threads>>>(d, 3, 5); break;
          case 12: rate<12><<<256, threads>>>(d, 3, 5); break;
          case 13: rate<13><<<256, threads>>>(d, 3, 5); break;
          case 14: rate<14><<<256, threads>>>(d, 3, 5); break;
          case 15: rate<15><<<256, threads>>>(d, 0xffffffffu, 5); break;
          case 16: rate<16><<<256, threads>>>(d, 3, 5); break;
          case 17: rate<17><<<256, threads>>>(d, 3, 5); break;
          case 18: rate<18><<<256, threads>>>(d, 3, 5); break;
          case 19: rate<19><<<256, threads>>>(d, 3, 5); break;
          case 20: rate<20><<<256, threads>>>(d, 3, 5); break;
          case 21: rate<21><<<256, threads>>>(d, 3, 5); break;
          case 22: rate<22><<<256, threads>>>(d, 3, 5); break;
          case 23: rate<23><<<256, threads>>>(d, 3, 5); break;
          case 24: rate<24><<<256, threads>>>(d, 3, 5); break;
          case 25: rate<25><<<256, threads>>>(d, 3, 5); break;
          case 26: rate<26><<<256, threads>>>(d, 3, 5); break;
          case 27: rate<27><<<256, threads>>>(d, 3, 0x00ff00ff); break;
          case 28: rate<28><<<256, threads>>>(d, 3, 0x00ff00ff); break;
          case 29: rate<29><<<256, threads>>>(d, 3, 5); break;
          case 30: rate<30><<<256, threads>>>(d, 3, 5); break;
          case 31: rate<31><<<256, threads>>>(d, 3, 5); break;
          case 32: rate<32><<<256, threads>>>(d, 0x1ff7c, 0x100fc); break;
          case 33: rate<33><<<256, threads>>>(d, 3, 5); break;
        }
        CK(hipDeviceSynchronize());
      }
      const int nw = 256 * 4 * waves;
      CK(hipMemcpy(h, d, nw * 8, hipMemcpyDeviceToHost));
      double s = 0;
      for (int i = 0; i < nw; i++) s += h[i];
      s /= nw;
      const double instr = 32.0 * kIters;                    // per wave
      const double cyc = s / instr;
      if (k == 0) base = s;
      printf("waves/SIMD %d  %-16s ~%.2f cycles per wave-instruction per wave (x%.2f v_add)  => SIMD %.2f cyc/instr\n",
             waves, names[k], cyc, s / base, cyc / waves);
    }
  }
  return 0;
}
