// learn_img.hpp -- the blocked LDS activation image of the 16-bit learn kernels
// (learn_h16.hpp, learn_shared.hip): its addressing and the transposed
// fragment read.
#pragma once

namespace dmdqn {

typedef short v4s __attribute__((vector_size(8)));
typedef __attribute__((address_space(3))) v4s lds_v4s;

// The activation images -- [128][128] H1, H2, dZ2, dZ1, the W2^T image and
// the [128][96] X -- are stored in 8-row x 32-column blocks of 512 B (a band
// of 8 rows is LD/32 blocks, a multiple of 256 B),
// row r's 16-byte chunks within a block XOR-permuted by bit 1 and bit 3 of r
// (a search over the linear permutations of row bits 0, 1, 3):
//   * row-fragment reads (ds_read_b128 of rows r0..r0+15, chunk 4s+lg): each
//     16-lane bank group {0-3,12-15 | 20-27} covers all 16 bank slots;
//   * transposed reads (ds_read_b64_tr_b16 of rows r0+8g+q, chunks 2c..2c+1):
//     each 32-lane half covers all 32 eight-byte slots;
// so both are conflict-free (the plain 256-B rows were 8-way on both), the
// 8-byte MFMA-output stores are 2-way (the least any permutation of whole
// 16-byte chunks allows for 16 rows at one column), and
// every address is a lane constant plus an immediate.  (The 2-way conflicts
// of the 192-B X rows go too.)  tests/test_layout_cpu.py restates it.
template <int LD = 128>
__device__ __forceinline__ int hoff(int r, int c) {
    static_assert(LD % 32 == 0, "whole blocks per band");
    const int ch = c >> 3;
    return 8 * LD * (r >> 3) + 256 * (ch >> 2) + 32 * (r & 7) +
           8 * ((ch & 3) ^ (((r >> 1) & 1) | ((r >> 2) & 2))) + (c & 7);
}

// Two ds_read_b64_tr_b16 at p0 and p0 + stride (elements), repacked to 8
// values.  Lane 4q+p of each 16-lane group addresses row q, columns 4p..4p+3
// of a 4-row block; lane i receives column i of the block (row q -> element
// q), the second read's rows in elements 4..7.
template <typename T>
__device__ __forceinline__ auto frag_tr2(const T *p0, int stride) {
    typedef T vec8 __attribute__((ext_vector_type(8)));
    v4s t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s *)p0);
    v4s t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s *)(p0 + stride));
    vec8 r;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        r[e] = __builtin_bit_cast(T, (short)t0[e]);
        r[e + 4] = __builtin_bit_cast(T, (short)t1[e]);
    }
    return r;
}

}  // namespace dmdqn
