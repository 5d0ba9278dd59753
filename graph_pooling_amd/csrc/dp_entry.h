// Argument checks of every exported C entry: each check is defined here once, with its wording (DP_CHECK itself lives
// in dp_common.h beside set_error).  A source keeps only the checks whose wording or shape rule is its own, built on
// DP_CHECK.  Where several exported names run one op (plain / _w / batch, dense / packed) they forward to one checked
// body and pass their own name and wording; a refusal sets the error text and returns its code before any launch.
#pragma once
#include "dp_common.h"

namespace dp {

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The weighted-CSR rule of the _w entries: `values` is required; `values_t` only beside a transposed CSR of its own
// (indices_t given and not the forward's array).  Without one the forward's values serve both directions.
inline bool own_transpose(const int* indices, const int* indices_t) { return indices_t && indices_t != indices; }
inline const float* values_t_of(const int* indices, const int* indices_t, const float* values, const float* values_t) {
    return own_transpose(indices, indices_t) ? values_t : values;
}

}  // namespace dp

#define DP_STREAM(s) ((hipStream_t)(s))
// a check that is a function of its own (shape rules, host tables, the pending device error): the entry refuses with it
#define DP_TRY(call)                          \
    do {                                      \
        const int try_rc_ = (call);           \
        if (try_rc_ != DP_OK) return try_rc_; \
    } while (0)
// scalars: a count that must be there, one that may be zero, a leading dimension against the width it must cover
#define DP_POS(v) DP_CHECK((v) > 0, DP_ERR_INVALID_ARG, #v "=%d must be positive", (int)(v))
#define DP_NONNEG(v) DP_CHECK((v) >= 0, DP_ERR_INVALID_ARG, #v "=%d must not be negative", (int)(v))
#define DP_LD(ld, w) DP_CHECK((ld) >= (w), DP_ERR_INVALID_ARG, #ld "=%d smaller than its width %d", (int)(ld), (int)(w))
// a device (or host table) pointer of 4-byte elements: there and aligned
#define DP_NOTNULL(p) DP_CHECK((p) != nullptr, DP_ERR_INVALID_ARG, #p " is NULL")
#define DP_ALIGNED4(p) DP_CHECK(((uintptr_t)(p) & 3) == 0, DP_ERR_INVALID_ARG, #p " is not 4-byte aligned")
#define DP_PTR(p)       \
    do {                \
        DP_NOTNULL(p);  \
        DP_ALIGNED4(p); \
    } while (0)
#define DP_ALIGNED8(p) DP_CHECK(((uintptr_t)(p) & 7) == 0, DP_ERR_INVALID_ARG, #p " is not 8-byte aligned")
// 16-byte alignment (workspaces, packed planes); null_ok: NULL passes.  The wording is the entry's; _P: the fixed one.
#define DP_ALIGNED16(p, null_ok, ...) \
    DP_CHECK(((null_ok) || (p) != nullptr) && ::dp::aligned16(p), DP_ERR_INVALID_ARG, __VA_ARGS__)
#define DP_ALIGNED16_P(p) DP_ALIGNED16(p, true, #p " is not 16-byte aligned")
// values / values_t of a body with `weighted`, `indices`, `indices_t`, `values`, `values_t` in scope.  NULL is refused
// in the entry's wording (the message follows); `then` is the statement run on a pointer that is there: the entry's
// alignment check, or (void)0 where it has none
#define DP_VALUES(then, ...)                                                \
    do {                                                                    \
        if (weighted) {                                                     \
            DP_CHECK(values != nullptr, DP_ERR_INVALID_ARG, __VA_ARGS__);   \
            then;                                                           \
        }                                                                   \
    } while (0)
#define DP_VALUES_T(then, ...)                                              \
    do {                                                                    \
        if (weighted && ::dp::own_transpose(indices, indices_t)) {          \
            DP_CHECK(values_t != nullptr, DP_ERR_INVALID_ARG, __VA_ARGS__); \
            then;                                                           \
        }                                                                   \
    } while (0)
