// err.cc — error reporting and the environment switches' readers (err.h).
#include "err.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

namespace tips {
namespace rt {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  if (getenv("TIPS_VERBOSE")) fprintf(stderr, "[tips] error %d: %s\n", code, buf);
  return code;
}

const std::string& last_error() { return g_last_error; }

int64_t env_i64(const char* name, int64_t dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  return strtoll(v, nullptr, 10);
}

int env_first_int(const char* const* names, int dflt) {
  for (int i = 0; names[i]; i++) {
    const char* v = getenv(names[i]);
    if (v && *v) return atoi(v);
  }
  return dflt;
}

}  // namespace rt
}  // namespace tips
