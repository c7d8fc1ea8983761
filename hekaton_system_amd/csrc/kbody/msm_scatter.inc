// body of k_msm_scatter and its batched twin (msm.cuh, msm_batch.cuh): one source, so the single-proof kernel's code is unchanged
    __shared__ u32 h[MSM_LDS_COUNTERS];
    for (u32 b = threadIdx.x; b < p.NB; b += blockDim.x) h[b] = 0;
    __syncthreads();
    size_t base = (size_t)blockIdx.x * p.chunk;
    for (u32 k = threadIdx.x; k < p.chunk; k += blockDim.x) {
        size_t i = base + k;
        if (i >= p.n) break;
        for (u32 w = 0; w < p.W; w++) {
            int d = digits[(size_t)w * p.n + i];
            if (d != 0) atomicAdd(&h[(w % p.WP) * p.B + msm_mag(d) - 1], 1u);
        }
    }
    __syncthreads();
    // reserve this workgroup's range in every non-empty bucket; h[b] becomes the running position
    for (u32 b = threadIdx.x; b < p.NB; b += blockDim.x) {
        u32 v = h[b];
        if (v) h[b] = atomicAdd(&cursor[b], v);
    }
    __syncthreads();
    for (u32 k = threadIdx.x; k < p.chunk; k += blockDim.x) {
        size_t i = base + k;
        if (i >= p.n) break;
        for (u32 w = 0; w < p.W; w++) {
            int d = digits[(size_t)w * p.n + i];
            if (d != 0) {
                u32 pos = atomicAdd(&h[(w % p.WP) * p.B + msm_mag(d) - 1], 1u);
                sorted[pos] = ((w / p.WP) << p.gshift) | (u32)i | (d < 0 ? 0x80000000u : 0u);
            }
        }
    }
