// body of k_msm_accum_tail and its batched twin (msm.cuh, msm_batch.cuh): one source, so the single-proof kernel's code is unchanged
    u32 t = threadIdx.x;
    u32 E = start[p.NB];
    for (int level = level0; level < (int)p.n_levels; level++) {
        LevelInfo li = msm_level_info(p, E, level);
        bool in0 = ((level - 1) & 1) == 0;           // level k reads buffer (k-1)&1 and writes buffer k&1
        if (t < li.active)
            msm_accum_level<F>(level, t, li, in0 ? keys0 : keys1, in0 ? pts0 : pts1, p, buckets, in0 ? keys1 : keys0,
                               in0 ? pts1 : pts0);
        __threadfence_block();
        __syncthreads();
    }
