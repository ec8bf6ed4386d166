// gpx_env.h — every environment switch libgpx.so reads, defined once (host only).
//
// GPX_ENV_TABLE is the only definition of a switch: its name, the EnvKnobs field it fills, the field's kind, the moment
// it is read, its default (the value of an unset variable) and its validity rule (the value of a set one, an expression
// in `e`, the variable's text).  This header holds the library's only calls of getenv; INTEGRATION.md §7 is the
// user-facing copy of the table and tests/test_env_knobs.py holds the two together.
//
// The moments (EnvAt):
//   create   gpx_create fills the entry; it holds for the handle's lifetime.
//   call     the handle's snapshot (gpx_handle::env) is refreshed at the start of every extern "C" call that enqueues
//            work (begin_call and what shares it); everything the call runs — schedulers, rank threads' member
//            handles, a retry — reads that snapshot, never the environment.
//   process  read once, where it guards a dlopen (roctx(), rccl_api()); never part of a handle's snapshot.
//
// Kinds: Flag (bool; prints 0 / 1), Int, I64, Opt (int; a negative value is "unset" and prints so), Str (text or
// null; null prints "unset").
#ifndef GPX_ENV_H_
#define GPX_ENV_H_

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace gpx {

enum class EnvAt { create, call, process };

namespace env_rule {
inline bool flag(const char* e) { return atoi(e) != 0; }  // set: on unless it reads as 0 ("", "x" and "0" are off)
// a block width: a multiple of 128 in [128, hi], anything else is `otherwise`
inline int block(const char* e, int hi, int otherwise) {
  const int v = atoi(e);
  return (v >= 128 && v <= hi && v % 128 == 0) ? v : otherwise;
}
inline int64_t in_range(int64_t v, int64_t lo, int64_t hi, int64_t otherwise) { return (v >= lo && v <= hi) ? v : otherwise; }
}  // namespace env_rule

// X(name, field, kind, read at, default, rule)
#define GPX_ENV_TABLE(X)                                                                                               \
  /* the Cholesky schedule (chol_enqueue, diag_enqueue) */                                                             \
  X("GPX_DIAG_STEP", diag_step, Int, call, 128, atoi(e) == 64 ? 64 : 128)                                              \
  X("GPX_CHAIN_FLAG", chain_flag, Opt, call, -1, env_rule::flag(e))                                                    \
  X("GPX_FUSED_STRIP", fused_strip, Flag, call, false, env_rule::flag(e))                                              \
  X("GPX_SPLIT_STRIP", split_strip, Flag, call, true, env_rule::flag(e))                                               \
  X("GPX_SOLVE_TOP", solve_top, Flag, call, true, env_rule::flag(e))                                                   \
  X("GPX_REST_SPLIT", rest_split, Int, call, 16, atoi(e))                                                              \
  X("GPX_CU_SELF_RESERVE", cu_self_reserve, Int, call, 0, (int)env_rule::in_range(atoi(e), 1, 4, 0))                   \
  X("GPX_RESV_ALL", resv_all, Flag, call, false, env_rule::flag(e))                                                    \
  X("GPX_RESV_CHAIN", resv_chain, Int, call, 1, atoi(e))                                                               \
  X("GPX_RESV_FORM", resv_form, Int, call, 1, atoi(e))                                                                 \
  /* the two-level Cholesky (chol_two_level_enqueue) and its Strassen level (strassen_nt) */                           \
  X("GPX_TWO_LEVEL_FROM", two_level_from, I64, call, 65536, env_rule::in_range(atoll(e), 0, 1L << 40, 0))                  \
  X("GPX_STRASSEN_MIN", strassen_min, I64, call, 4096, env_rule::in_range(atoll(e), 0, 1L << 40, 0) / 128 * 128)          \
  X("GPX_STRASSEN_MIN_TWO", strassen_min2, I64, call, 4096, env_rule::in_range(atoll(e), 0, 1L << 40, 0) / 128 * 128)        \
  X("GPX_STRASSEN_DIAG", strassen_diag, Flag, call, false, env_rule::flag(e))                                          \
  X("GPX_STRASSEN_SINGLE", strassen_f32, Flag, call, false, env_rule::flag(e))                                            \
  X("GPX_DEFER_LEFT", defer_left, Opt, call, -1, env_rule::flag(e))                                                    \
  /* widths and batches */                                                                                          \
  X("GPX_NB_WIDE_FROM", nb_wide_from, I64, call, 40960, (int64_t)atoll(e))                                             \
  X("GPX_NB_GRAD", nb_grad, Int, call, 0, env_rule::block(e, 4096, 0))                                                 \
  X("GPX_NB_SOLVE", nb_solve, Int, create, 256, env_rule::block(e, 4096, 256))                                         \
  X("GPX_NB_PRED", nb_pred, Opt, create, -1, env_rule::block(e, 4096, 1024))                                           \
  X("GPX_NB_SHARD", nb_shard, Int, create, 0, env_rule::block(e, 2048, 0))                                             \
  X("GPX_PRED_BATCH", pred_batch, I64, call, 8192, env_rule::in_range(atol(e), 128, 1L << 22, 8192) / 128 * 128)       \
  X("GPX_FEW_SOLVE", few_solve, Flag, call, true, env_rule::flag(e))                                                   \
  /* shards and device groups */                                                                                       \
  X("GPX_SHARD_DEAL", shard_snake, Int, call, 1, (strcmp(e, "cyclic") == 0 || strcmp(e, "0") == 0) ? 0 : 1)            \
  X("GPX_SHARD_REPLICATE", shard_replicate, Opt, call, -1, env_rule::flag(e))                                          \
  X("GPX_SHARD_DENSE_PANEL", shard_dense_panel, Flag, call, true, env_rule::flag(e))                                   \
  X("GPX_SHARD_TWO_PIPE", shard_two_pipe, Opt, call, -1, env_rule::flag(e))                                            \
  X("GPX_SHARD_FUSED", shard_fused, Flag, call, true, env_rule::flag(e))                                               \
  X("GPX_REPL_COPY_SIDE", repl_copy_side, Flag, call, true, env_rule::flag(e))                                         \
  X("GPX_GROUP_INITALL", group_initall, Flag, call, true, env_rule::flag(e))                                           \
  X("GPX_LOCAL_FORCE_PEER", local_force_peer, Flag, call, false, env_rule::flag(e))                                    \
  /* diagnostics */                                                                                                    \
  X("GPX_MICROBENCH_ITERS", microbench_iters, Int, call, 65536, (int)env_rule::in_range(atol(e), 64, 1L << 20, 65536)) \
  X("GPX_ROCTX", roctx, Flag, process, true, env_rule::flag(e))                                                        \
  X("GPX_RCCL_PATH", rccl_path, Str, process, nullptr, e)

struct EnvKnobs {
  using Flag = bool;
  using Int = int;
  using I64 = int64_t;
  using Opt = int;
  using Str = const char*;  // the environment's own text: valid until the variable changes (process entries only)
#define GPX_ENV_FIELD(name, field, kind, at, dflt, rule) kind field = dflt;
  GPX_ENV_TABLE(GPX_ENV_FIELD)
#undef GPX_ENV_FIELD
  // foreign — read, not owned: rocprofv3 --pmc exports ROCPROF_COUNTER_COLLECTION=1 into the profiled process (read
  // with the call entries; not an entry of the table, not printed)
  bool counters_collected = false;
};

// fills the entries of the table that are read at `at`; the others keep their values
inline void env_read(EnvKnobs& k, EnvAt at) {
#define GPX_ENV_READ(name, field, kind, at_, dflt, rule) \
  if (at == EnvAt::at_) {                                \
    const char* e = getenv(name);                        \
    k.field = e ? (rule) : (dflt);                       \
  }
  GPX_ENV_TABLE(GPX_ENV_READ)
#undef GPX_ENV_READ
  if (at == EnvAt::call) {
    const char* e = getenv("ROCPROF_COUNTER_COLLECTION");
    k.counters_collected = e && atoi(e) != 0;
  }
}

// One "NAME=value\n" line per entry of the table into buf (at most n - 1 characters and a terminating 0; nothing when
// buf is null or n <= 0).  Returns the length of the whole text, as snprintf does.
inline int env_print(const EnvKnobs& k, char* buf, int n) {
  int len = 0;
  auto put = [&](const char* name, const char* fmt, auto v) {
    const bool room = buf && n > 0 && len < n;
    const int w = snprintf(room ? buf + len : nullptr, room ? (size_t)(n - len) : 0, fmt, name, v);
    if (w > 0) len += w;
  };
  // one printer per kind, NAMED as the kind column of the table (and as EnvKnobs' type aliases): GPX_ENV_PRINT picks it by that name
  auto Flag = [&](const char* name, bool v) { put(name, "%s=%d\n", (int)v); };
  auto Int = [&](const char* name, int v) { put(name, "%s=%d\n", v); };
  auto I64 = [&](const char* name, int64_t v) { put(name, "%s=%lld\n", (long long)v); };
  auto Opt = [&](const char* name, int v) { v < 0 ? put(name, "%s=%s\n", "unset") : put(name, "%s=%d\n", v); };
  auto Str = [&](const char* name, const char* v) { put(name, "%s=%s\n", v ? v : "unset"); };
#define GPX_ENV_PRINT(name, field, kind, at, dflt, rule) kind(name, k.field);
  GPX_ENV_TABLE(GPX_ENV_PRINT)
#undef GPX_ENV_PRINT
  return len;
}

}  // namespace gpx

#endif  // GPX_ENV_H_
