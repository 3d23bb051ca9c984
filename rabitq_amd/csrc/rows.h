// rows.h -- the row types of an index (RQ_ROWS_* of include/rabitq_hip.h), each question about one answered once: RowSpec.  Included
// by common.h, so host and device code see the same answers.  A new row type, or a change to what one allows, belongs here.
//
// Half-precision rows (RQ_ROWS_F16 = 1, RQ_ROWS_BF16 = 2): the index stores the caller's 2-byte elements as given, 2*dim bytes per row,
// never tiered, never split, no shadow rows.  Widening W to f32 is exact (f16: the IEEE conversion, subnormals kept; bf16:
// bits << 16), so every distance is the f32 index's of W(rows), bit for bit.
// Byte rows (RQ_ROWS_U8 = 4, RQ_ROWS_I8 = 5): the caller's one-byte elements as given, dim bytes per row, padding 0x00, never tiered,
// never split, no shadow rows.  W(u8) = the integer as f32, W(i8) = the two's-complement integer as f32: both exact, so every
// distance is the f32 index's of W(rows), bit for bit.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/rabitq_hip.h"

// W of one stored byte, and its inverse on representable values (anything else: clamped and truncated -- the loaders check with
// narrow_exact, host_build.h, before they store)
__host__ __device__ __forceinline__ float rq_widen_byte(uint8_t b, uint32_t fmt) {
    return fmt == RQ_ROWS_I8 ? (float)(int32_t)(int8_t)b : (float)(uint32_t)b;
}
__host__ __device__ __forceinline__ uint8_t rq_narrow_byte(float v, uint32_t fmt) {
    if (fmt == RQ_ROWS_I8) return (uint8_t)(int8_t)(int32_t)(v >= 127.0f ? 127.0f : v >= -128.0f ? v : -128.0f);  // (a NaN: -128)
    return (uint8_t)(uint32_t)(v >= 255.0f ? 255.0f : v >= 0.0f ? v : 0.0f);                                        // (a NaN: 0)
}
// W of one stored 2-byte element
__host__ __device__ __forceinline__ float rq_widen_elem(uint16_t h, uint32_t fmt) {
    if (fmt == RQ_ROWS_BF16) return __builtin_bit_cast(float, (uint32_t)h << 16);
#ifdef __HIP_DEVICE_COMPILE__
    return (float)__builtin_bit_cast(_Float16, h);
#else
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, ex = (h >> 10) & 31u, man = h & 0x3FFu;
    if (ex == 31u) return __builtin_bit_cast(float, sign | 0x7F800000u | (man ? 0x00400000u | (man << 13) : 0u));
    if (ex != 0u) return __builtin_bit_cast(float, sign | ((ex + 112u) << 23) | (man << 13));
    const float mag = (float)man * 5.9604644775390625e-8f;  // man * 2^-24: exact
    return sign ? -mag : mag;
#endif
}
// R_t of one f32 value: round to nearest even to the storage type (f16: subnormal results kept, overflow to inf; bf16:
// (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the bits u).  A NaN stays a NaN, and one whose low 16 bits are zero keeps its bf16 bits.
__host__ __device__ __forceinline__ uint16_t rq_narrow_elem(float v, uint32_t fmt) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    if (fmt == RQ_ROWS_BF16) {
        if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | ((u & 0xFFFFu) ? 0x40u : 0u));
        return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
    }
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_bit_cast(uint16_t, (_Float16)v);
#else
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return (uint16_t)(sign | 0x7E00u | ((a >> 13) & 0x3FFu));
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);  // >= 65520 rounds to inf (inf itself included)
    if (a < 0x33000001u) return (uint16_t)sign;               // <= 2^-25 rounds to zero (the tie goes to the even 0)
    const uint32_t e = a >> 23;
    // 24-bit significand shifted so that the result counts units of the target's last place (normal: 2^(e-127-10), subnormal: 2^-24)
    const uint32_t sig = (a & 0x7FFFFFu) | 0x800000u, sh = e >= 113u ? 13u : 126u - e;
    const uint32_t q = sig >> sh, rem = sig & ((1u << sh) - 1u), halfway = 1u << (sh - 1u);
    const uint32_t r = q + ((rem > halfway || (rem == halfway && (q & 1u))) ? 1u : 0u);
    // normal: q carries the hidden bit (0x400 .. 0x7FF), so adding (e - 113) << 10 lands the exponent, and a carry out of the
    // significand moves into it; subnormal: r is the significand itself (a carry to 0x400 is the smallest normal)
    return (uint16_t)(sign | (e >= 113u ? ((e - 113u) << 10) + r : r));
#endif
}

// f32 / 2-byte / one-byte elements: what the kernels that read an index's rows are instantiated on (kernels_rerank.h:
// accurate_rows<KIND>); which of the two types of its kind a row holds stays a run-time field
enum { ROW_KIND_F32 = 0, ROW_KIND_HALF = 1, ROW_KIND_BYTE = 2 };

// One row type.  `id` is the RQ_ROWS_* value: what rq_index stores, and what BaseView::fmt / RowRef::fmt carry to the kernels as a
// plain uint32_t.
struct RowSpec {
    uint32_t id = RQ_ROWS_F32;
    __host__ __device__ __forceinline__ bool known() const { return id <= RQ_ROWS_BF16 || id == RQ_ROWS_U8 || id == RQ_ROWS_I8; }
    __host__ __device__ __forceinline__ bool typed() const { return id != RQ_ROWS_F32; }  // the caller's elements are stored as given
    __host__ __device__ __forceinline__ bool bytes() const { return id >= RQ_ROWS_U8; }
    __host__ __device__ __forceinline__ int kind() const { return id == RQ_ROWS_F32 ? ROW_KIND_F32 : bytes() ? ROW_KIND_BYTE : ROW_KIND_HALF; }
    __host__ __device__ __forceinline__ uint32_t elem_bytes() const { return id == RQ_ROWS_F32 ? 4u : bytes() ? 1u : 2u; }
    __host__ __device__ __forceinline__ size_t row_bytes(uint32_t dim) const { return (size_t)dim * elem_bytes(); }
    // f32 slots (4 bytes) one stored row of dim elements takes: the stride of BaseView::dev
    __host__ __device__ __forceinline__ uint32_t row_slots(uint32_t dim) const { return id == RQ_ROWS_F32 ? dim : bytes() ? dim >> 2 : dim >> 1; }
    // W of element i of `p` (elements of this type), and R_t(v) stored there (a typed spec; f32 elements are read and written as they are)
    __host__ __device__ __forceinline__ float widen(const void *p, uint64_t i) const {
        return bytes() ? rq_widen_byte(static_cast<const uint8_t *>(p)[i], id) : rq_widen_elem(static_cast<const uint16_t *>(p)[i], id);
    }
    __host__ __device__ __forceinline__ void narrow(void *p, uint64_t i, float v) const {
        if (bytes()) static_cast<uint8_t *>(p)[i] = rq_narrow_byte(v, id);
        else static_cast<uint16_t *>(p)[i] = rq_narrow_elem(v, id);
    }
    // The metrics a row type goes with: the inner product has no typed rows (its extra coordinate sqrt(S - |x|^2) is not a value of
    // the type), the cosine metric no byte rows (nor is a normalised row).  Every entry and both loaders ask here; each words its
    // own refusal.
    bool allowed_with(uint32_t metric) const { return !typed() || (metric != RQ_METRIC_IP && !(bytes() && metric == RQ_METRIC_COSINE)); }
    // the stored tag of a typed spec: the `rows` file of a dumped directory ("f16\n" / "bf16\n" / "u8\n" / "i8\n"), the "rows" member
    // of a JSON dump
    const char *tag() const { return id == RQ_ROWS_U8 ? "u8" : id == RQ_ROWS_I8 ? "i8" : id == RQ_ROWS_BF16 ? "bf16" : "f16"; }
    static bool from_tag(const char *text, size_t len, RowSpec *out) {
        const uint32_t ids[] = {RQ_ROWS_F16, RQ_ROWS_BF16, RQ_ROWS_U8, RQ_ROWS_I8};
        for (uint32_t id : ids)
            if (len == strlen(RowSpec{id}.tag()) && memcmp(text, RowSpec{id}.tag(), len) == 0) return *out = RowSpec{id}, true;
        return false;
    }
};
