// err.h — the calling thread's last error and the environment switches' readers: what every
// translation unit of the runtime needs, and all that the HIP-free ones do (neg_protocol.cc).
#pragma once

#include <stdint.h>

#include <string>

namespace tips {
namespace rt {

// Records the calling thread's last error (tips_last_error) and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
const std::string& last_error();

#define TRY(expr)            \
  do {                       \
    int rc_ = (expr);        \
    if (rc_ != 0) return rc_; \
  } while (0)

int64_t env_i64(const char* name, int64_t dflt);
int env_first_int(const char* const* names, int dflt);

}  // namespace rt
}  // namespace tips
