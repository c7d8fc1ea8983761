// body of k_msm_hist and its batched twin (msm.cuh, msm_batch.cuh): one source, so the single-proof kernel's code is unchanged
    __shared__ u32 h[MSM_LDS_COUNTERS];
    for (u32 b = threadIdx.x; b < p.NB; b += blockDim.x) h[b] = 0;
    __syncthreads();
    size_t base = (size_t)blockIdx.x * p.chunk;
    for (u32 k = threadIdx.x; k < p.chunk; k += blockDim.x) {
        size_t i = base + k;
        if (i >= p.n) break;
        u32 sp[10];
        msm_load_scalar<Fr>(scalars, i, is_mont, p, sp);
        for (u32 w = 0; w < p.W; w++) {
            int d = msm_digit(sp, w, p.c);
            // the signed digits are computed ONCE per scalar (Montgomery reduction + split) and kept, window-major,
            // for the two passes of k_msm_scatter: 2 bytes per digit, coalesced across the lanes of a wave
            digits[(size_t)w * p.n + i] = (short)d;
            if (d != 0) {
                u32 mag = d < 0 ? (u32)(-d) : (u32)d;
                atomicAdd(&h[(w % p.WP) * p.B + mag - 1], 1u);
            }
        }
    }
    __syncthreads();
    for (u32 b = threadIdx.x; b < p.NB; b += blockDim.x) {
        u32 v = h[b];
        if (v) atomicAdd(&count[b], v);
    }
