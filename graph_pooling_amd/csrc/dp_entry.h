// Argument checks of the exported C entries, shared by the CSR / ragged sources and the CSR part of dp_api.hip.
// An exported name forwards to one checked body per op and passes its own name for the messages; a refusal sets the
// error text and returns its code before anything is launched.
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

#define DP_CHECK(cond, code, ...)         \
    do {                                  \
        if (!(cond)) {                    \
            ::dp::set_error(__VA_ARGS__); \
            return code;                  \
        }                                 \
    } while (0)
// a device (or host table) pointer of 4-byte elements: there and aligned
#define DP_NOTNULL(p) DP_CHECK((p) != nullptr, DP_ERR_INVALID_ARG, #p " is NULL")
#define DP_ALIGNED4(p) DP_CHECK(((uintptr_t)(p) & 3) == 0, DP_ERR_INVALID_ARG, #p " is not 4-byte aligned")
#define DP_PTR(p)       \
    do {                \
        DP_NOTNULL(p);  \
        DP_ALIGNED4(p); \
    } while (0)
// 16-byte alignment (workspaces, packed planes); null_ok: NULL passes.  The wording is the entry's.
#define DP_ALIGNED16(p, null_ok, ...) \
    DP_CHECK(((null_ok) || (p) != nullptr) && ::dp::aligned16(p), DP_ERR_INVALID_ARG, __VA_ARGS__)
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
