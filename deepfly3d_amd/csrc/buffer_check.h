// The buffer rules every a15 entry applies before it touches the device (the rules of a14, behaviour_segment.hip): no null pointer, the
// alignment the kernels' accesses need, and no two buffers of one call sharing a byte.  The message names the argument.
#pragma once
#include <cstdint>

#include "common.h"

namespace df3d {

struct Range {
    const char* name;
    const void* ptr;
    long long bytes;
    int align;
};

inline int check_buffers(const char* fn, const Range* r, int count) {
    for (int a = 0; a < count; ++a) {
        if (!r[a].ptr) {
            set_error("%s: null pointer: %s", fn, r[a].name);
            return DF3D_EINVAL;
        }
        if ((uintptr_t)r[a].ptr & (uintptr_t)(r[a].align - 1)) {
            set_error("%s: %s must be %d-byte aligned", fn, r[a].name, r[a].align);
            return DF3D_EINVAL;
        }
    }
    for (int a = 0; a < count; ++a)
        for (int b = a + 1; b < count; ++b) {
            const char *pa = static_cast<const char*>(r[a].ptr), *pb = static_cast<const char*>(r[b].ptr);
            if (pa < pb + r[b].bytes && pb < pa + r[a].bytes) {
                set_error("%s: %s must not overlap %s", fn, r[b].name, r[a].name);
                return DF3D_EINVAL;
            }
        }
    return DF3D_OK;
}

#define DF3D_BUFFERS(...)                                                                                                   \
    do {                                                                                                                    \
        const df3d::Range ranges__[] = {__VA_ARGS__};                                                                       \
        if (const int rc__ = df3d::check_buffers(__func__, ranges__, (int)(sizeof(ranges__) / sizeof(df3d::Range)))) return rc__; \
    } while (0)

}  // namespace df3d
