// The prologue shared by the fp32-MFMA convolution kernels (included from conv_mfma.h): where a workgroup's tile lies (the XCD-aware
// remap itself is raft_xcd_remap in launch_plan.h, checked on the host), the buffer descriptors of the sources and the weights, the
// staging of a halo tile -- item table, global load of a K chunk, LDS store with the optional fused PRE -- and the weight-fragment
// fetch.  What stays in the kernels is their own geometry (tile and halo shape, LDS placement of a halo pixel, which K quad a
// fragment row is) and the order in which the main loop issues these pieces.
//
// Addressing rule, as in conv_epilogue.h: every load is an unconditional buffer load; an item outside the image gets RAFT_OOB as its
// byte offset and the descriptor's bounds check answers 0.
#pragma once

// ---- descriptors.  A source is [Min][ld] floats of which channels [0, c) are read: (Min - 1) * ld + c floats.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raft_stage_rsrc(const void *base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, bytes, 0x00020000);
}
// first source, built unconditionally (c: p.c0, or 4 for the stem's padded image)
__device__ __forceinline__ int raft_stage_src0_bytes(const ConvArgs &p, int Min, int c) { return (int)((((long)Min - 1) * p.lda0 + c) * 4); }
// second source; absent (c1 = 0): an empty descriptor on a0
__device__ __forceinline__ const float *raft_stage_src1_base(const ConvArgs &p) { return p.c1 ? p.a1 : p.a0; }
__device__ __forceinline__ int raft_stage_src1_bytes(const ConvArgs &p, int Min) { return p.c1 ? (int)((((long)Min - 1) * p.lda1 + p.c1) * 4) : 0; }
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raft_stage_src0(const ConvArgs &p, int Min, int c) {
    return raft_stage_rsrc(p.a0, raft_stage_src0_bytes(p, Min, c));
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raft_stage_src1(const ConvArgs &p, int Min) {
    return raft_stage_rsrc(raft_stage_src1_base(p), raft_stage_src1_bytes(p, Min));
}
// weights packed [taps][cin / 4][npad][4]
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raft_stage_weights(const ConvArgs &p, int taps, int cin) {
    return raft_stage_rsrc(p.wp, (int)((long)taps * cin * p.npad * 4));
}

// ---- staging item table.  Item tid + NTHR * i of a thread = (halo pixel hp = (hy, hx) of an HH x HWP tile, 16-byte channel quad c4 of
// QS): pix[i] = its input pixel (image b of Hi x Wi, halo origin (yorg, xorg), `step` input pixels between halo pixels) or -1 outside
// the image and for the padding items behind the tile; lds_off[i] = place(hp, hy, hx) + c4 in 16-byte units, `dummy` for padding items.
// Scalars come in by const reference: by value (`noundef` to hipcc) 11 F(2x2) instances change register or spill counts (NOTEBOOK 25).
template <int NTHR, int QS, int HWP, int HP, int NA, class Place>
__device__ __forceinline__ void raft_stage_items(const int &tid, const int &b, const int &Hi, const int &Wi, const int &yorg, const int &xorg,
                                                 const int &step, Place place, const int &dummy, int (&pix)[NA], int (&lds_off)[NA]) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int item = tid + NTHR * i;
        const int hp = item / QS, c4 = item % QS;
        const int hy = hp / HWP, hx = hp - hy * HWP;
        const int yy = yorg + hy * step, xx = xorg + hx * step;
        const bool ok = (hp < HP) & ((unsigned)yy < (unsigned)Hi) & ((unsigned)xx < (unsigned)Wi);
        pix[i] = ok ? (b * Hi + yy) * Wi + xx : -1;
        lds_off[i] = hp < HP ? place(hp, hy, hx) + c4 : dummy;
    }
}

// ---- global load of the K chunk that starts at channel ch of the concatenated sources (a chunk never straddles them); quad = the
// thread's 16-byte channel quad inside the chunk.  One branch per chunk, not per load (conv_mfma.h: unconditional loads).
template <int NA>
__device__ __forceinline__ void raft_stage_gload(const ConvArgs &p, __amdgpu_buffer_rsrc_t rs0, __amdgpu_buffer_rsrc_t rs1, const int (&pix)[NA],
                                                 int ch, int quad, f32x4 (&ra)[NA]) {
    const bool first = ch < p.c0;
    const int ld = first ? p.lda0 : p.lda1;
    const int chl = (first ? ch : ch - p.c0) + quad * 4;
    if (first) {
#pragma unroll
        for (int i = 0; i < NA; ++i) ra[i] = raft_buffer_load_f4(rs0, pix[i] >= 0 ? (unsigned)((pix[i] * ld + chl) * 4) : RAFT_OOB);
    } else {
#pragma unroll
        for (int i = 0; i < NA; ++i) ra[i] = raft_buffer_load_f4(rs1, pix[i] >= 0 ? (unsigned)((pix[i] * ld + chl) * 4) : RAFT_OOB);
    }
}
// PRE: scale / shift of the thread's channel quad of that chunk, image b
__device__ __forceinline__ void raft_stage_pre_load(const ConvArgs &p, int b, int cin, int ch, int quad, f32x4 &sc, f32x4 &sh) {
    sc = *(const f32x4 *)(p.pre_scale + (long)b * cin + ch + quad * 4);
    sh = *(const f32x4 *)(p.pre_shift + (long)b * cin + ch + quad * 4);
}

// ---- LDS store of the staged chunk into the buffer at `buf`; PRE applies relu(x * scale + shift) to in-image items (padding stays zero)
template <int PRE, int NA>
__device__ __forceinline__ void raft_stage_lstore(float *buf, const int (&lds_off)[NA], const int (&pix)[NA], const f32x4 (&ra)[NA],
                                                  const f32x4 &pre_sc, const f32x4 &pre_sh) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        f32x4 v = ra[i];
        if (PRE) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = pix[i] >= 0 ? fmaxf(fmaf(v[e], pre_sc[e], pre_sh[e]), 0.f) : 0.f;
        }
        *(f32x4 *)(buf + lds_off[i] * 4) = v;
    }
}
template <int NA>
__device__ __forceinline__ void raft_stage_lstore(float *buf, const int (&lds_off)[NA], const f32x4 (&ra)[NA]) {
    raft_stage_lstore<0>(buf, lds_off, lds_off, ra, ra[0], ra[0]);
}

// ---- weight fragments straight from L2: lane (k-quad G, channel n0 + wave_n + LR: tile, wave's first channel in it, lane) of the
// packed layout, TN column blocks of 16 channels from row (tap t, k-quad kq) -- wave-uniform, in the instruction's scalar operand.
// The sum keeps this order: with the channel added up first, six F(2x2) and 25 direct instances come out with other SGPR-spill
// counts (docs/NOTEBOOK.md 25).
__device__ __forceinline__ unsigned raft_stage_b_lane(const ConvArgs &p, int G, int n0, int wave_n, int LR) {
    return (unsigned)(((G * p.npad) + n0 + wave_n + LR) * 16);   // bytes
}
template <int TN>
__device__ __forceinline__ void raft_stage_frag_b(const ConvArgs &p, __amdgpu_buffer_rsrc_t rsw, unsigned b_lane, int cin, int t, int kq, f32x4 *bf) {
    const unsigned row = (unsigned)((t * (cin >> 2) + kq) * p.npad) * 16u;   // wave-uniform bytes
#pragma unroll
    for (int j = 0; j < TN; ++j)
        bf[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsw, (int)(b_lane + j * 256), (int)row, 0));
}
