// body of k_msm_scan and its batched twin (msm.cuh, msm_batch.cuh): one source, so the single-proof kernel's code is unchanged
    __shared__ u32 part[1024];
    u32 per = (NB + 1023) / 1024;
    u32 lo = threadIdx.x * per, hi = min(lo + per, NB);
    u32 s = 0;
    for (u32 b = lo; b < hi; b++) s += count[b];
    part[threadIdx.x] = s;
    __syncthreads();
    // Hillis-Steele inclusive scan over 1024 partials
    for (u32 off = 1; off < 1024; off <<= 1) {
        u32 v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    u32 run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (u32 b = lo; b < hi; b++) {
        start[b] = run;
        cursor[b] = run;
        run += count[b];
    }
    if (threadIdx.x == 1023) start[NB] = part[1023];
