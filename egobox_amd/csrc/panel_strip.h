// The strip arithmetic of every panel solve (gfx950), device only: ONE body for
//     the strip solve    X_k = T_k Linv_k^T,  under the tile's refinement flag followed by  X += (T - X L_kk^T) Linv_k^T
//     the strip update   T_C -= X_k L(C, k)^T
// on 16x16 tiles held as FP64-MFMA accumulators (lane (frow, fk), register q <-> T[frow][4 fk + q]: the convention of
// potf2_blocks.h, where the operand layouts and the refinement step are derived).
// CONTRACT.  Every kernel that solves a panel -- the TRSM slots of rb_factor_block (potf2_blocks.h), k_panel_trsm16 and
// k_panel_trsm_rows (kernels_chol.hip), pipe_role_trsm (kernels_pipe.hip) -- forms X with rb_strip_solve (+ rb_strip_refine)
// and applies it with rb_strip_update, from fragments masked by rb_mask_lower and read at row rb_prow(frow); nothing else forms X or applies
// it.  A tile therefore meets the same instructions on the same values in the same order (updates for k ascending, then
// the solve) whichever kernel owns it: the launch forms give the same bits by construction.  What a kernel adds is who owns
// which tile, what is staged or prefetched when, and the hand-offs.
#pragma once
#include <hip/hip_runtime.h>

namespace egx {

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double d2_t __attribute__((ext_vector_type(2)));

constexpr int RB_LD = 18;  // LDS row stride (doubles): b128 reads of 16 rows hit 16 distinct 4-bank groups

// one 16x16x16 product on the matrix cores: c +-= A' B' with both operands as 4 consecutive doubles per lane.  NEG = 1
// negates A' in the instruction (the FP64 MFMAs of gfx940+ read their BLGP field as neg:[a,b,c]).
#define RB_MFMA4(c, NEG, a01, a23, b0, b1, b2, b3)                               \
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(a01[0], b0, c, 0, 0, NEG);           \
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(a01[1], b1, c, 0, 0, NEG);           \
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(a23[0], b2, c, 0, 0, NEG);           \
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(a23[1], b3, c, 0, 0, NEG)

// a write-through (sc1) store for the in-launch hand-offs, see potf2_blocks.h
__device__ __forceinline__ void store_d2_sc1(double *p, d2_t v) {
    // (inline asm is invisible to the hazard recogniser: the TWO wait states gfx940+ needs between a store of more than 64
    //  bits and a VALU write of its data registers are part of the statement -- with one, a v_and that followed the asm
    //  replaced the low word of a stored double in lanes 0..15)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}
template <bool SC1>
__device__ __forceinline__ void store_d2(double *p, d2_t v) {
    if constexpr (SC1) store_d2_sc1(p, v);
    else *reinterpret_cast<d2_t *>(p) = v;
}

// pi(i) = 4 (i % 4) + i / 4: the matrix row whose fragment lane row `frow` supplies as the A' operand
__device__ __forceinline__ int rb_prow(int frow) { return ((frow & 3) << 2) | (frow >> 2); }

// a lane's four doubles of a tile, at p = &T[frow][4 fk] (global or LDS)
__device__ __forceinline__ double4_t rb_load4(const double *p) {
    const d2_t v0 = *reinterpret_cast<const d2_t *>(p), v1 = *reinterpret_cast<const d2_t *>(p + 2);
    return double4_t{v0[0], v0[1], v1[0], v1[1]};
}
template <bool SC1 = false>
__device__ __forceinline__ void rb_store4(double *p, double4_t v) {
    store_d2<SC1>(p, d2_t{v[0], v[1]});
    store_d2<SC1>(p + 2, d2_t{v[2], v[3]});
}

// the fragments of L_kk (row prow, columns col .. col + 3, col = 4 fk) as the A' operand of X L_kk^T: zero right of the diagonal
__device__ __forceinline__ void rb_mask_lower(d2_t &r01, d2_t &r23, int prow, int col) {
    r01 = d2_t{(col <= prow) ? r01[0] : 0.0, (col + 1 <= prow) ? r01[1] : 0.0};
    r23 = d2_t{(col + 2 <= prow) ? r23[0] : 0.0, (col + 3 <= prow) ? r23[1] : 0.0};
}

// X = T Linv^T (n01 / n23: row pi(frow) of Linv_k)
__device__ __forceinline__ double4_t rb_strip_solve(double4_t tile, d2_t n01, d2_t n23) {
    double4_t x = double4_t{0.0, 0.0, 0.0, 0.0};
    RB_MFMA4(x, 0, n01, n23, tile[0], tile[1], tile[2], tile[3]);
    return x;
}
// one step of iterative refinement, X += (T - X L_kk^T) Linv^T, on the masked fragments l01 / l23 of L_kk; the residual
// is formed in the tile's own registers (the tile is dead once it has become X)
__device__ __forceinline__ void rb_strip_refine(double4_t &x, double4_t &tile, d2_t n01, d2_t n23, d2_t l01, d2_t l23) {
    RB_MFMA4(tile, 1, l01, l23, x[0], x[1], x[2], x[3]);
    RB_MFMA4(x, 0, n01, n23, tile[0], tile[1], tile[2], tile[3]);
}
// the solve of a strip whose masked fragments are at hand: the refinement step under the tile's flag.  (A kernel that
// fetches or masks them under the flag only calls the two halves itself, the step inside its own branch.)
__device__ __forceinline__ double4_t rb_strip_solve(double4_t tile, d2_t n01, d2_t n23, d2_t l01, d2_t l23, bool refine) {
    double4_t x = rb_strip_solve(tile, n01, n23);
    if (refine) rb_strip_refine(x, tile, n01, n23, l01, l23);
    return x;
}

// T_C -= X_k L(C, k)^T (a01 / a23: row pi(frow) of L(C, k)); also T -= X X^T with X's own rows pi(frow) as a01 / a23
__device__ __forceinline__ void rb_strip_update(double4_t &tile, d2_t a01, d2_t a23, double4_t x) {
    RB_MFMA4(tile, 1, a01, a23, x[0], x[1], x[2], x[3]);
}
// ... with the fragments read where they lie, a = &L(C, k)[pi(frow)][4 fk] (LDS or global)
__device__ __forceinline__ void rb_strip_update(double4_t &tile, const double *a, double4_t x) {
    rb_strip_update(tile, *reinterpret_cast<const d2_t *>(a), *reinterpret_cast<const d2_t *>(a + 2), x);
}

}  // namespace egx
