// witness_host.cuh — assignments built on the device: bit expansion, word programs and Poseidon Merkle paths (kernels in
// witness.cuh; the membership walk in poseidon.cuh).  Defines Ops<C>::assignment_from_bits (hk_assignment_from_bits), wprog_upload / wprog_free / wprog_run
// (hk_wprog_*), assignment_scatter (hk_assignment_scatter), poseidon_path (hk_poseidon_path).
#pragma once
#include "curve_ops_impl.cuh"
#include "job_args.h"
#include "poseidon.cuh"
#include "witness.cuh"

namespace hk {

// z[i] = bits[i] ? 1 : 0 (Montgomery), then z[full_cols[k]] = full_vals[k]
template <class Fr>
__global__ void k_expand_bits(const unsigned char* __restrict__ bits, size_t n, Fr* __restrict__ z) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fr_store(&z[i], bits[i] ? Fr::one() : Fr::zero());
}
template <class Fr>
__global__ void k_scatter_full(const u32* __restrict__ cols, const Fr* __restrict__ vals, u32 k, size_t n, Fr* __restrict__ z) {
    u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    u32 c = cols[j];
    if (c < n) fr_store(&z[c], fr_load(&vals[j]));
}

template <class C>
hk_status Ops<C>::assignment_from_bits(hk_ctx* ctx, const void* bits, size_t n_v, const uint32_t* full_cols,
                                       const void* full_vals, size_t n_full, void* z_out) {
    if (n_v == 0) return HK_OK;
    if (!is_device_ptr(z_out)) return HK_ERR_ARG;
    Staged in[3] = {staged(bits, n_v), staged(full_cols, 4 * n_full), staged(full_vals, sizeof(Fr) * n_full)};
    if (in[1].scratch)                                      // host columns are checked here; resident ones by the kernel
        for (size_t k = 0; k < n_full; k++) if (full_cols[k] >= n_v) return HK_ERR_ARG;
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    HK_TRY(L->carve([&](Carve& c) { stage_carve(c, in, 3); }));
    HK_TRY(stage_upload(L, in, 3));
    HK_LAUNCH((k_expand_bits<Fr>), dim3((u32)((n_v + 255) / 256)), dim3(256), 0, L->stream, (const unsigned char*)in[0].p,
              n_v, (Fr*)z_out);
    if (n_full)
        HK_LAUNCH((k_scatter_full<Fr>), dim3((u32)((n_full + 63) / 64)), dim3(64), 0, L->stream, (const u32*)in[1].p,
                  (const Fr*)in[2].p, (u32)n_full, n_v, (Fr*)z_out);
    return L->settle();
}

// ---- word programs (witness.cuh) ---------------------------------------------------------------------------------
template <class C>
hk_status Ops<C>::wprog_upload(hk_ctx* ctx, const uint32_t* ops, size_t n_ops, const uint32_t* refs, size_t n_refs,
                               const uint32_t* map, size_t n_v, size_t n_values, size_t n_inputs, hk_wprog** out) {
    *out = nullptr;
    if (n_values >= (1u << 20) || n_ops == 0 || n_v == 0 || n_v >= ((size_t)1 << 32)) return HK_ERR_ARG;
    // validate on the host what the interpreter will index with: operand references, operand tables, the column map
    size_t vid = 0;
    auto ref_ok = [&](uint32_t r) { return (r & 0xfffffu) < vid; };
    for (size_t k = 0; k < n_ops; k++) {
        const uint32_t* o = ops + 8 * k;
        bool ok = true;
        switch (o[0]) {
            case WOP_INPUT: ok = o[4] < n_inputs; break;
            case WOP_CONST: break;
            case WOP_XOR: case WOP_AND: ok = ref_ok(o[1]) && ref_ok(o[2]); break;
            case WOP_CH: case WOP_MAJ: ok = ref_ok(o[1]) && ref_ok(o[2]) && ref_ok(o[3]); break;
            case WOP_ADD:
                ok = (size_t)o[1] + o[2] <= n_refs && o[2] <= 16;
                for (uint32_t j = 0; ok && j < o[2]; j++) ok = ref_ok(refs[o[1] + j]);
                vid++;
                break;
            case WOP_PACK4:
                ok = (size_t)o[1] + 4 <= n_refs;
                for (uint32_t j = 0; ok && j < 4; j++) ok = ref_ok(refs[o[1] + j]);
                break;
            case WOP_SHA_ROUND: case WOP_SHA_SCHED: {
                const uint32_t nr = o[0] == WOP_SHA_ROUND ? 9u : 4u;
                ok = (size_t)o[1] + nr <= n_refs;
                for (uint32_t j = 0; ok && j < nr; j++) ok = ref_ok(refs[o[1] + j]);
                vid += (o[0] == WOP_SHA_ROUND ? WOP_ROUND_VALUES : WOP_SCHED_VALUES) - 1;
                break;
            }
            default: ok = false;
        }
        if (!ok) return HK_ERR_ARG;
        vid++;
    }
    if (vid != n_values) return HK_ERR_ARG;
    for (size_t i = 0; i < n_v; i++)
        if (map[i] != 0xffffffffu && (map[i] >> 5) >= n_values) return HK_ERR_ARG;
    HK_HIP(hipSetDevice(ctx->device));
    WprogImpl* w = new WprogImpl();
    hk_wprog* h = new hk_wprog{ctx->ops, ctx, w};
    auto fail = [&](hk_status st) { Ops<C>::wprog_free(h); return st; };
    auto up = [&](u32** dst, const uint32_t* src, size_t n) -> bool {
        if (hipMalloc((void**)dst, 4 * (n ? n : 1)) != hipSuccess) { (void)hipGetLastError(); return false; }
        return n == 0 || hipMemcpy(*dst, src, 4 * n, hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!up(&w->ops, ops, 8 * n_ops) || !up(&w->refs, refs, n_refs) || !up(&w->map, map, n_v)) return fail(HK_ERR_NOMEM);
    w->n_ops = (u32)n_ops; w->n_refs = (u32)n_refs; w->n_values = (u32)n_values; w->n_inputs = (u32)n_inputs; w->n_v = n_v;
    *out = h;
    return HK_OK;
}

template <class C>
void Ops<C>::wprog_free(hk_wprog* h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipDeviceSynchronize();
    for (u32* p : {h->impl->ops, h->impl->refs, h->impl->map}) if (p) (void)hipFree(p);
    delete h->impl;
    delete h;
}

template <class C>
hk_status Ops<C>::wprog_run(hk_ctx* ctx, const hk_wprog* h, const uint32_t* inputs, size_t batch,
                            const uint32_t* full_cols, const void* full_vals, size_t n_full, void* z_out) {
    const WprogImpl* w = h->impl;
    if (batch == 0) return HK_OK;
    if (batch >= (1u << 16) || !is_device_ptr(z_out)) return HK_ERR_ARG;
    Staged in[3] = {staged(inputs, 4 * batch * w->n_inputs), staged(full_cols, 4 * n_full),
                    staged(full_vals, sizeof(Fr) * n_full * batch)};
    if (in[1].scratch)                                      // host columns are checked here; resident ones by the kernel
        for (size_t k = 0; k < n_full; k++) if (full_cols[k] >= w->n_v) return HK_ERR_ARG;
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    u32* values;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, in, 3);
        values = c.n<u32>((size_t)w->n_values * batch);
    }));
    hipStream_t s = L->stream;
    const void *in_d = in[0].p, *cd = in[1].p, *vd = in[2].p;
    HK_TRY(stage_upload(L, in, 3));
    HK_LAUNCH((k_word_program<0>), dim3((u32)((batch + 63) / 64)), dim3(64), 0, s, w->ops, w->n_ops, w->refs,
              (const u32*)in_d, w->n_inputs, (u32)batch, values);
    HK_LAUNCH((k_witness_expand<Fr>), dim3((u32)((w->n_v + 255) / 256), (u32)batch), dim3(256), 0, s, w->map, w->n_v,
              (const u32*)values, (u32)batch, (Fr*)z_out);
    if (n_full)
        HK_LAUNCH((k_scatter_full_batch<Fr>), dim3((u32)((n_full + 63) / 64), (u32)batch), dim3(64), 0, s,
                  (const u32*)cd, (const Fr*)vd, (u32)n_full, w->n_v, (Fr*)z_out);
    return L->settle();
}

// z_out[b][full_cols[j]] = full_vals[b][j]: the full-width values alone, for a caller that ran the class's word program
// earlier (hk_wprog_run with n_full = 0) and learns the values that depend on the round's challenges later
template <class C>
hk_status Ops<C>::assignment_scatter(hk_ctx* ctx, const uint32_t* full_cols, const void* full_vals, size_t n_full, size_t batch,
                                     size_t n_v, void* z_out) {
    if (batch == 0 || n_full == 0) return HK_OK;
    if (batch >= (1u << 16) || !is_device_ptr(z_out)) return HK_ERR_ARG;
    Staged in[2] = {staged(full_cols, 4 * n_full), staged(full_vals, sizeof(Fr) * n_full * batch)};
    if (in[0].scratch)                                      // as hk_wprog_run
        for (size_t k = 0; k < n_full; k++) if (full_cols[k] >= n_v) return HK_ERR_ARG;
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    HK_TRY(L->carve([&](Carve& c) { stage_carve(c, in, 2); }));
    const void *cd = in[0].p, *vd = in[1].p;
    HK_TRY(stage_upload(L, in, 2));
    HK_LAUNCH((k_scatter_full_batch<Fr>), dim3((u32)((n_full + 63) / 64), (u32)batch), dim3(64), 0, L->stream,
              (const u32*)cd, (const Fr*)vd, (u32)n_full, n_v, (Fr*)z_out);
    return L->settle();
}

template <class C>
hk_status Ops<C>::poseidon_path(hk_ctx* ctx, const void* consts, size_t n_consts, const hk_poseidon_desc* lh,
                                const hk_poseidon_desc* nh, const void* leaf, const void* siblings, const uint32_t* index,
                                size_t depth, size_t batch, size_t n_v, size_t col0, void* z_out) {
    if (batch == 0) return HK_OK;
    if (!consts || !lh || !nh || !leaf || !index || (depth && !siblings) || !is_device_ptr(z_out)) return HK_ERR_ARG;
    if (batch >= (1u << 20) || depth > 32) return HK_ERR_ARG;
    for (const hk_poseidon_desc* d : {lh, nh}) {
        if (d->t < 2 || d->t > 4 || (d->alpha != 5 && d->alpha != 17) || (d->full_rounds & 1) ||
            (size_t)d->consts_offset + (size_t)(d->full_rounds + d->partial_rounds) * d->t + (size_t)d->t * d->t > n_consts)
            return HK_ERR_ARG;
    }
    // the kernel is compiled for the reference's two instances (poseidon_util.rs:53-62): rate 3 / x^5 over the 4 leaf
    // fields, rate 2 / x^17 for two-to-one; round counts and constants stay run-time data
    if (lh->t != 4 || nh->t != 3 || lh->alpha != 5 || nh->alpha != 17) return HK_ERR_ARG;
    size_t block = poseidon_path_len(lh, nh, depth);
    if (col0 > n_v || block > n_v - col0) return HK_ERR_ARG;
    Staged in[4] = {staged(consts, n_consts * sizeof(Fr)), staged(leaf, batch * 4 * sizeof(Fr)),
                    staged(siblings, batch * depth * sizeof(Fr)), staged(index, 4 * batch)};
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    HK_TRY(L->carve([&](Carve& c) { stage_carve(c, in, 4); }));
    const void *cd = in[0].p, *ld = in[1].p, *sd = in[2].p, *id = in[3].p;
    HK_TRY(stage_upload(L, in, 4));
    // row b is its own source: leaf b, path b, direction bits from index[b]
    HK_TRY((poseidon_membership<Fr, 4>(L->stream, cd, lh, nh, ld, sd, nullptr, (const u32*)id, 1, depth, batch, n_v, col0, z_out)));
    return L->settle();
}

}  // namespace hk
