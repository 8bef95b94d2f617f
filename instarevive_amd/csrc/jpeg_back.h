// The back half of libjpeg's decoder as device functions: the ISLOW inverse DCT of jidctint.c, the fancy chroma upsampling of jdsample.c and the
// constants of the colour conversion. degrade.hip (the JPEG round trip of ir_degrade) and jpeg_decode.hip (ir_jpeg_decode) share them, so that
// both are the same arithmetic, held to Pillow byte for byte. Integers only: nothing here depends on the floating-point contraction flags.
#pragma once
#include "common.h"

namespace ir_jpeg_back {

IR_DEVINL int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
constexpr int FIX(double x) { return (int)(x * 65536.0 + 0.5); }

typedef long long i64;
constexpr i64 F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299, F_1_847 = 15137,
              F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;
IR_DEVINL i64 descale(i64 x, int n) { return (x + ((i64)1 << (n - 1))) >> n; }

template <bool FIRST>
IR_DEVINL void idct8(i64 d[8]) {   // jidctint.c, one column (FIRST) or one row
    constexpr int N = FIRST ? 13 - 2 : 13 + 2 + 3;
    i64 z1 = (d[2] + d[6]) * F_0_541;
    i64 t2 = z1 + d[6] * (-F_1_847), t3 = z1 + d[2] * F_0_765;
    i64 t0 = (d[0] + d[4]) * 8192, t1 = (d[0] - d[4]) * 8192;
    const i64 t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
    z1 = t0 + t3;
    i64 z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const i64 z5 = (z3 + z4) * F_1_175;
    t0 *= F_0_298, t1 *= F_2_053, t2 *= F_3_072, t3 *= F_1_501;
    z1 *= -F_0_899, z2 *= -F_2_562, z3 *= -F_1_961, z4 *= -F_0_390;
    z3 += z5, z4 += z5;
    t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
    d[0] = descale(t10 + t3, N), d[7] = descale(t10 - t3, N);
    d[1] = descale(t11 + t2, N), d[6] = descale(t11 - t2, N);
    d[2] = descale(t12 + t1, N), d[5] = descale(t12 - t1, N);
    d[3] = descale(t13 + t0, N), d[4] = descale(t13 - t0, N);
}

// h2v2 fancy upsampling of a chroma plane with rows of CW bytes whose true size is ch x cw.
// 3 * near + far of chroma column cx for output row y (the row above the first and below the last is the edge row itself)
IR_DEVINL int chroma_v(const uint8_t* __restrict__ C, int CW, int ch, int y, int cx) {
    const int cy = y >> 1, far = (y & 1) ? (cy + 1 < ch ? cy + 1 : ch - 1) : (cy > 0 ? cy - 1 : 0);
    return 3 * (int)C[cy * CW + cx] + (int)C[far * CW + cx];
}

IR_DEVINL int chroma_up(const uint8_t* __restrict__ C, int CW, int ch, int cw, int y, int x) {
    const int cx = x >> 1, cs = chroma_v(C, CW, ch, y, cx);
    if (x & 1) return (3 * cs + (cx + 1 < cw ? chroma_v(C, CW, ch, y, cx + 1) : cs) + 7) >> 4;
    return (3 * cs + (cx > 0 ? chroma_v(C, CW, ch, y, cx - 1) : cs) + 8) >> 4;
}

// h2v1 fancy upsampling: the first and the last output column of the true chroma width cw copy their sample
IR_DEVINL int chroma_up_h(const uint8_t* __restrict__ row, int cw, int x) {
    const int cx = x >> 1, c = row[cx];
    if (x & 1) return cx + 1 < cw ? (3 * c + (int)row[cx + 1] + 2) >> 2 : c;
    return cx > 0 ? (3 * c + (int)row[cx - 1] + 1) >> 2 : c;
}

}  // namespace ir_jpeg_back
