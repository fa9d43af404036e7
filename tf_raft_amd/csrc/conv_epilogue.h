// The epilogue shared by the fp32-MFMA convolution kernels (included from conv_mfma.h): buffer descriptors of the output /
// gate operands, per-lane channel bookkeeping, the value formulas of every ConvEpilogue code and the STATS tail.  What stays
// in the kernels is their own geometry -- which pixel a register holds, the output transform of a Winograd family, when the
// gate inputs are fetched -- and their ablation hooks.
//
// Addressing rule of all of them: stores and loads are unconditional buffer accesses; a lane (or element) that takes no part
// gets RAFT_OOB as (or or-ed into) its byte offset, which the descriptor's bounds check drops / answers with 0.
#pragma once

__device__ __forceinline__ float raft_buffer_load_f32(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, int soff = 0) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, soff, 0));
}
__device__ __forceinline__ void raft_buffer_store_f32(float v, __amdgpu_buffer_rsrc_t rsrc, unsigned voff, int soff = 0) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc, (int)voff, soff, 0);
}

// Descriptor of an [M][ld] operand of which columns [0, w) are touched: (M - 1) * ld + w floats.  An absent operand gets a
// zero-sized descriptor on `fallback` (always p.o0, which is never null): every load through it returns 0.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raft_epi_rsrc(const void *ptr, const void *fallback, bool present, int M, int ld, int w) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)(present ? ptr : fallback), 0, present ? (int)((((long)M - 1) * ld + w) * 4) : 0,
                                             0x00020000);
}

struct EpiBuffers {
    __amdgpu_buffer_rsrc_t o0, o1, e0, e1;
};
// GRU_ZR splits its nvalid = hid + (nvalid - hid) channels over o0 (z) and o1 (r * h) and reads h = e0 for the second part;
// every other code writes nvalid columns of o0.  e0: GRU_ZR, GRU_Q (h), RES (the block input); e1: GRU_Q (z).
template <int EPI>
__device__ __forceinline__ EpiBuffers raft_epi_buffers(const ConvArgs &p, int M) {
    constexpr bool has_e0 = EPI == EPI_GRU_ZR || EPI == EPI_GRU_Q || EPI == EPI_RES, has_e1 = EPI == EPI_GRU_Q;
    const int w0 = (EPI == EPI_GRU_ZR) ? p.hid : p.nvalid;          // valid columns of o0, and of e0 / e1
    const int w1 = (EPI == EPI_GRU_ZR) ? p.nvalid - p.hid : 0;      // valid columns of o1
    return {raft_epi_rsrc(p.o0, p.o0, true, M, p.ldo0, w0), raft_epi_rsrc(p.o1, p.o0, w1 > 0, M, p.ldo1, w1),
            raft_epi_rsrc(p.e0, p.o0, has_e0, M, p.lde0, w0), raft_epi_rsrc(p.e1, p.o0, has_e1, M, p.lde1, w0)};
}
// the accumulator preload / context addend `init` (NULL: zero-sized, loads give 0)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raft_epi_init_buffer(const ConvArgs &p, int M) {
    return raft_epi_rsrc(p.init, p.o0, p.init != nullptr, M, p.ldi, p.nvalid);
}

// What output channel n of a lane means to the epilogue: nok = a real channel (n < nvalid); isz = in the z half of GRU_ZR;
// nh = its column in o0 / o1 / e0 (n, or n - hid in the r half of GRU_ZR); to0 .. te1 = the lane's channel touches that operand.
// Used by the Winograd families.  The direct kernel (conv_halo.h) spells the same predicates out in its own text: built from
// these member functions its GRU gate instances come out with other register and spill counts (docs/NOTEBOOK.md 20).
template <int EPI>
struct EpiChannel {
    static constexpr bool ZR = EPI == EPI_GRU_ZR, HAS_E0 = ZR || EPI == EPI_GRU_Q || EPI == EPI_RES;
    const ConvArgs &p;
    const int n;
    __device__ __forceinline__ EpiChannel(const ConvArgs &p_, int n_) : p(p_), n(n_) {}
    __device__ __forceinline__ bool nok() const { return n < p.nvalid; }
    __device__ __forceinline__ bool isz() const { return n < p.hid; }
    __device__ __forceinline__ unsigned nh() const { return (unsigned)(ZR ? (isz() ? n : n - p.hid) : n); }
    __device__ __forceinline__ bool to0() const { const bool k = nok(), z = isz(); return ZR ? (k & z) : k; }
    __device__ __forceinline__ bool to1() const { const bool k = nok(), z = isz(); return ZR && (k & !z); }
    __device__ __forceinline__ bool te0() const { const bool k = nok(), z = isz(); return HAS_E0 && (ZR ? (k & !z) : k); }
    __device__ __forceinline__ bool te1() const { return EPI == EPI_GRU_Q && nok(); }
};
// Lane byte bases of (pixel pix0, the lane's channel) in each operand, RAFT_OOB where the channel takes no part; the kernels
// add a wave-uniform element offset in the instruction's scalar operand and or in the element's out-of-image bit.
struct EpiBases {
    unsigned o0, o1, e0, e1, init;
};
template <int EPI>
__device__ __forceinline__ EpiBases raft_epi_bases(const ConvArgs &p, const EpiChannel<EPI> &c, unsigned pix0) {
    return {c.to0() ? (pix0 * p.ldo0 + c.nh()) * 4u : RAFT_OOB, c.to1() ? (pix0 * p.ldo1 + c.nh()) * 4u : RAFT_OOB,
            c.te0() ? (pix0 * p.lde0 + c.nh()) * 4u : RAFT_OOB, c.te1() ? (pix0 * p.lde1 + c.n) * 4u : RAFT_OOB,
            c.nok() ? (pix0 * p.ldi + c.n) * 4u : RAFT_OOB};
}

// Output value of every code but GRU_ZR from v = accumulator (+ init) + bias.  The library is built with -ffp-contract=on,
// which contracts within one expression: each formula is ONE expression so that the same FMAs form in every kernel.
// Floats come in by const reference here and in the STATS tail: a by-value float parameter tells hipcc that the caller's
// value is no poison, the epilogue loops of the direct kernel are then unswitched differently and kernels at the edge of a
// register budget (the STATS tiles of the encoders, the F(2x2) gate kernel) move by a few registers.
template <int EPI>
__device__ __forceinline__ float raft_epi_act(const float &v0, const float &e0, const float &e1, const float &scale) {
    float v = v0;
    if constexpr (EPI == EPI_GRU_Q) {
        const float q = raft_tanh(v);
        return (1.0f - e1) * e0 + e1 * q;                 // h <- (1 - z) h + z q: e0 = h, e1 = z
    } else if constexpr (EPI == EPI_RES) {
        return fmaxf(e0 + fmaxf(v, 0.f), 0.f);            // ResBlock tail: e0 = the block's input
    } else {
        static_assert(EPI == EPI_LINEAR || EPI == EPI_RELU, "GRU_ZR has two outputs: raft_epi_gate_zr");
        if (EPI == EPI_RELU) v = fmaxf(v, 0.f);
        return v * scale;
    }
}
// GRU_ZR: a lane of the z half stores *z to o0, one of the r half *rh = r * h to o1 (the other store is out of range)
__device__ __forceinline__ void raft_epi_gate_zr(float v, float h, float *z, float *rh) {
    *z = raft_sigmoid(v);
    *rh = *z * h;
}

// STATS tail: lanes LR, LR + 16, LR + 32, LR + 48 hold partial (sum, sum of squares) of the same channel n; lane group 0
// stores the total as entry `entry` of p.stats[entry][npad][2]
__device__ __forceinline__ void raft_epi_stats_store(const ConvArgs &p, const float &sum, const float &sumsq, int G, long entry, int n) {
    float s1 = sum, s2 = sumsq;
    s1 += __shfl_xor(s1, 16, 64);
    s2 += __shfl_xor(s2, 16, 64);
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    if (G == 0) *(float2 *)(p.stats + (entry * p.npad + n) * 2) = make_float2(s1, s2);
}
