// The library's environment variables (config.h): the only file under csrc that reads the environment.
#include "config.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <string>

#include "../../include/cora_hip.h"

namespace cora {
namespace {

enum class Kind { Flag, Int, Real };
enum class Life { Once, Call };

struct Entry {
  const char *name;
  Kind kind;
  Life life;
  long double dflt, lo, hi;  // (long double holds every int64_t exactly)
  const char *description;
};

constexpr Entry kTable[] = {
#define CORA_ENV_ENTRY(id, name, kind, dflt, lo, hi, life, desc) \
  {name, Kind::kind, Life::life, static_cast<long double>(dflt), static_cast<long double>(lo), static_cast<long double>(hi), desc},
    CORA_ENV_TABLE(CORA_ENV_ENTRY)
#undef CORA_ENV_ENTRY
};
constexpr int kCount = static_cast<int>(sizeof(kTable) / sizeof(kTable[0]));

struct Value {
  bool set;
  long double v;
};

Value read(const Entry &t) {
  const char *e = std::getenv(t.name);
  if (!e) return {false, t.dflt};
  switch (t.kind) {
    case Kind::Flag: return {true, (e[0] != '\0' && e[0] != '0') ? 1.0L : 0.0L};
    case Kind::Int: return {true, std::clamp(static_cast<long double>(std::atoll(e)), t.lo, t.hi)};
    default: return {true, std::clamp(static_cast<long double>(std::stod(e)), t.lo, t.hi)};
  }
}

Value get(Env id) {
  const int i = static_cast<int>(id);
  const Entry &t = kTable[i];
  if (t.life == Life::Call) return read(t);
  static std::once_flag once[kCount];
  static Value cached[kCount];
  std::call_once(once[i], [&] { cached[i] = read(t); });
  return cached[i];
}

}  // namespace

bool env_flag(Env e) { return get(e).v != 0; }
int64_t env_int(Env e) { return static_cast<int64_t>(get(e).v); }
double env_real(Env e) { return static_cast<double>(get(e).v); }
bool env_set(Env e) { return get(e).set; }

}  // namespace cora

int cora_debug_config(char *buf, int len) {
  std::string out;
  for (int i = 0; i < cora::kCount; ++i) {
    out += std::string(cora::kTable[i].name) + "=";
    try {
      const cora::Value v = cora::get(static_cast<cora::Env>(i));
      char num[64];
      if (cora::kTable[i].kind == cora::Kind::Real)
        std::snprintf(num, sizeof(num), "%.17g", static_cast<double>(v.v));
      else
        std::snprintf(num, sizeof(num), "%lld", static_cast<long long>(v.v));
      out += std::string(num) + (v.set ? "" : " (default)") + "\n";
    } catch (const std::exception &) {  // (a real that std::stod rejects)
      out += "(not a number)\n";
    }
  }
  if (buf && len > 0) {
    const size_t n = std::min(out.size(), static_cast<size_t>(len) - 1);
    std::memcpy(buf, out.data(), n);
    buf[n] = '\0';
  }
  return static_cast<int>(out.size());
}
