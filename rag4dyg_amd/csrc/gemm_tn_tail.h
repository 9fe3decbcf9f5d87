// The tail of gemm_s3tn_kernel and gemm_b1tn_kernel, included as TEXT behind the k-loop (no include guard; gemm_tn_common.h says
// why text): the slice's column sums of dY through LDS, then the slice's partial tile.  Uses the kernels' locals: lds, cs, do_cs,
// dbp, acc, g, Cg, tid, lane, wi, wj, i0, j0 and the tile constants.
    if (do_cs) {                                                      // thread (token row t16 = tid >> 5, chunk tid & 31): 16 rows per chunk
        float* red = reinterpret_cast<float*>(lds);                  // the last iteration's barrier has passed: the stages are free
#pragma unroll
        for (int e = 0; e < 8; ++e) red[(tid >> 5) * 256 + (tid & 31) * 8 + e] = cs[e];
        __syncthreads();
        if (tid < 256) {
            float sum = 0.f;
#pragma unroll
            for (int t16 = 0; t16 < 16; ++t16) sum += red[t16 * 256 + tid];
            dbp[(size_t)blockIdx.z * g.J + j0 + tid] = sum;
        }
    }
    // partial tile of slice z (whole tiles only: I % 128 == 0, J % 256 == 0)
    float* C = Cg + (size_t)blockIdx.z * g.I * g.J;
    const int li = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + wi * WI + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, col = j0 + wj * WJ + j * 32 + li;
                C[(size_t)row * g.J + col] = acc[i][j][r];
            }
