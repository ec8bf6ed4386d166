// gpx_group.inc — single-process multi-GPU: a handle created with gpx_config.ndev > 1 is a
// GROUP of per-device member handles (SURVEY.md §8b "Threading": "Multi-GPU = single process,
// one stream set per device ... stays a drop-in for a plain Python caller").  Included by
// gpx_api.hip after gpx_shard.inc (same translation unit).
//
// Every group call (fit / predict) runs the row-block-cyclic schedule of gpx_shard.inc with one
// host thread per rank: rank 0 on the calling thread, ranks 1..P-1 on std::threads that live for
// the duration of the call.  The members talk through one of two transports:
//   RCCL   one communicator per device inside the process (ncclCommInitAll; GPX_GROUP_INITALL=0: P
//          grouped ncclCommInitRank calls on one unique id), each driven by its rank's thread on
//          that rank's streams (devices must be distinct);
//   LOCAL  LocalComm (gpx_shard.inc): peer copies + hipEvents, no library besides HIP; also
//          valid with a device listed several times, which is how the tests run 2..8 ranks
//          on the one GPU of the development box.
// The reference has no counterpart (one script, one thread: GPmap.py:163,212,220).

namespace {

struct Group {
  std::vector<gpx_handle*> members;
  LocalHub hub;
  int transport = GPX_TRANSPORT_LOCAL;
};

// Run f(member, rank) on every rank; returns the first genuine failure (a rank that only saw
// the abort of a peer reports GPX_E_COMM: prefer the peer's own error).
template <typename F>
int run_group(gpx_handle* g, F&& f) {
  Group* G = g->group;
  const int P = (int)G->members.size();
  G->hub.reset();
  std::vector<int> rc((size_t)P, GPX_OK);
  std::vector<std::thread> th;
  bool spawn_failed = false;
  try {
    th.reserve((size_t)P);
    for (int i = 1; i < P; ++i)
      th.emplace_back([&rc, &f, G, i] {
        rc[(size_t)i] = f(G->members[(size_t)i], i);
        if (rc[(size_t)i] != GPX_OK) G->hub.abort();
      });
  } catch (...) {
    spawn_failed = true;
    G->hub.abort();
  }
  if (!spawn_failed) {
    rc[0] = f(G->members[0], 0);
    if (rc[0] != GPX_OK) G->hub.abort();
  }
  for (auto& t : th) t.join();
  if (spawn_failed) return fail(g, GPX_E_NOMEM, "device group: could not start the rank threads");
  int first = -1;
  for (int i = 0; i < P; ++i)
    if (rc[(size_t)i] != GPX_OK && (first < 0 || (rc[(size_t)first] == GPX_E_COMM && rc[(size_t)i] != GPX_E_COMM)))
      first = i;
  if (first < 0) return GPX_OK;
  try {
    g->err = "rank " + std::to_string(first) + " (device " +
             std::to_string(G->members[(size_t)first]->cfg.device) + "): " + G->members[(size_t)first]->err;
  } catch (...) {
  }
  return rc[(size_t)first];
}

void destroy_group(gpx_handle* g) {
  Group* G = g->group;
  if (!G) return;
  for (gpx_handle* m : G->members)
    if (m) gpx_destroy(m);
  delete G;
  g->group = nullptr;
}

int create_group(gpx_handle** out, const gpx_config* cfg) {
  const int P = cfg->ndev;
  if (cfg->world != 1 || cfg->rank != 0)
    return fail(nullptr, GPX_E_ARG, "gpx_create: a device group (ndev > 1) needs rank = 0, world = 1");
  if (cfg->transport != GPX_TRANSPORT_AUTO && cfg->transport != GPX_TRANSPORT_RCCL &&
      cfg->transport != GPX_TRANSPORT_LOCAL)
    return fail(nullptr, GPX_E_ARG, "gpx_create: unknown group transport");
  bool distinct = true;
  for (int i = 0; i < P; ++i)
    for (int j = 0; j < i; ++j)
      if (cfg->devices[i] == cfg->devices[j]) distinct = false;
  int transport = cfg->transport;
  if (transport == GPX_TRANSPORT_AUTO) transport = distinct ? GPX_TRANSPORT_RCCL : GPX_TRANSPORT_LOCAL;
  if (transport == GPX_TRANSPORT_RCCL && !distinct)
    return fail(nullptr, GPX_E_ARG, "gpx_create: RCCL needs distinct devices (use GPX_TRANSPORT_LOCAL)");
  gpx_handle* g = new (std::nothrow) gpx_handle();
  Group* G = new (std::nothrow) Group();
  if (!g || !G) {
    delete g;
    delete G;
    return fail(nullptr, GPX_E_NOMEM, "gpx_create: out of host memory");
  }
  g->cfg = *cfg;
  g->group = G;
  refresh_env(g);  // (GPX_GROUP_INITALL below)
  G->transport = transport;
  int rc = GPX_OK;
  try {
    G->hub.init(P);
    G->members.assign((size_t)P, nullptr);
  } catch (...) {
    rc = fail(nullptr, GPX_E_NOMEM, "gpx_create: out of host memory");
  }
  for (int i = 0; i < P && rc == GPX_OK; ++i) {
    gpx_config mc = *cfg;
    mc.ndev = 0;
    mc.device = cfg->devices[i];
    mc.rank = i;
    mc.world = P;
    rc = gpx_create(&G->members[(size_t)i], &mc);  // leaves its message in g_create_error
    if (rc == GPX_OK) {
      G->members[(size_t)i]->in_group = true;
      G->members[(size_t)i]->discard_out = i > 0;
      G->hub.dev[(size_t)i] = mc.device;
    }
  }
  if (rc == GPX_OK) {
    // peer access both ways (an error = same device or already on), whatever the transport: a
    // caller's device pointer lives on ONE of the group's devices and every rank copies from it
    for (int i = 0; i < P; ++i)
      for (int j = 0; j < P; ++j)
        if (cfg->devices[i] != cfg->devices[j] && hipSetDevice(cfg->devices[i]) == hipSuccess) {
          (void)hipDeviceEnablePeerAccess(cfg->devices[j], 0);
          (void)hipGetLastError();
        }
  }
  if (rc == GPX_OK && transport == GPX_TRANSPORT_LOCAL) {
    for (int i = 0; i < P && rc == GPX_OK; ++i) {
      LocalComm* c = new (std::nothrow) LocalComm();
      if (!c) {
        rc = fail(nullptr, GPX_E_NOMEM, "gpx_create: out of host memory");
        break;
      }
      c->hub = &G->hub;
      c->rank = i;
      c->world = P;
      G->members[(size_t)i]->comm = c;
    }
  } else if (rc == GPX_OK) {
    std::string err;
    RcclApi* api = rccl_api(&err);
    void* comms[GPX_MAX_GROUP] = {};
    int devs[GPX_MAX_GROUP];
    for (int i = 0; i < P; ++i) devs[i] = cfg->devices[i];
    if (!api) {
      rc = fail(nullptr, GPX_E_COMM, err.c_str());
    } else {
      // One communicator per device, created from this thread: ncclCommInitAll (default), or P grouped
      // ncclCommInitRank calls on one unique id (GPX_GROUP_INITALL=0) — the creation style of the
      // one-process-per-GPU shard (gpx_comm_init).  Both are exercised by the one-rank group tests.
      int nrc = 0;
      const char* what = "ncclCommInitAll";
      if (g->env.group_initall) {
        nrc = api->CommInitAll(comms, P, devs);
      } else {
        what = "grouped ncclCommInitRank";
        Id128 id;
        nrc = api->GetUniqueId(&id);
        if (nrc == 0) nrc = api->GroupStart();
        if (nrc == 0) {
          int inner = 0;
          for (int i = 0; i < P && inner == 0; ++i) {
            if (hipSetDevice(devs[i]) != hipSuccess) inner = 1;  // ncclUnhandledCudaError
            if (inner == 0) inner = api->CommInitRank(&comms[i], P, id, i);
          }
          const int endrc = api->GroupEnd();
          nrc = inner != 0 ? inner : endrc;
        }
      }
      if (nrc != 0) {
        try {
          g_create_error = std::string(what) + " failed: " + api->GetErrorString(nrc);
        } catch (...) {
        }
        rc = GPX_E_COMM;
      }
    }
    for (int i = 0; i < P && rc == GPX_OK; ++i) {
      RcclComm* c = new (std::nothrow) RcclComm();
      if (!c) {
        rc = fail(nullptr, GPX_E_NOMEM, "gpx_create: out of host memory");
        break;
      }
      c->api = api;
      c->comm = comms[i];
      comms[i] = nullptr;
      c->rank = i;
      c->world = P;
      G->members[(size_t)i]->comm = c;
    }
    if (rc != GPX_OK && api)
      for (int i = 0; i < P; ++i)
        if (comms[i]) api->CommDestroy(comms[i]);
  }
  if (rc != GPX_OK) {
    destroy_group(g);
    delete g;
    return rc;
  }
  *out = g;
  return GPX_OK;
}

int group_fit(gpx_handle* g, const void* X, const void* y, int64_t N, int32_t d, int32_t k,
              const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter,
              int32_t mem_kind, int64_t* info) {
  Group* G = g->group;
  std::vector<int64_t> infos(G->members.size(), 0);
  g->fitted = false;
  g->err.clear();
  const int rc = run_group(g, [&](gpx_handle* m, int r) {
    return gpx_fit(m, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, mem_kind, &infos[(size_t)r]);
  });
  if (rc != GPX_OK) return rc;
  *info = infos[0];  // the all-reduce(min) inside shard_fit made it the same on every rank
  g->fitted = (*info == 0);
  return GPX_OK;
}

// gpx_fit_predict on a group: every member takes its slice of the query points through its part of the sharded
// factorisation (gpx_fit_predict on the member handles: collective); rank 0 delivers the gathered result.
int group_fit_predict(gpx_handle* g, const void* X, const void* y, int64_t N, int32_t d, int32_t k,
                      const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter, const void* Xq,
                      int64_t M, void* mean, void* var, int32_t mem_kind, int64_t* info) {
  Group* G = g->group;
  std::vector<int64_t> infos(G->members.size(), 0);
  g->fitted = false;
  g->err.clear();
  const int rc = run_group(g, [&](gpx_handle* m, int r) {
    return gpx_fit_predict(m, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, Xq, M, mean, var, mem_kind,
                           &infos[(size_t)r]);
  });
  if (rc != GPX_OK) return rc;
  *info = infos[0];
  g->fitted = (*info == 0);
  return GPX_OK;
}

int group_predict(gpx_handle* g, const void* Xq, int64_t M, void* mean, void* var, int32_t mem_kind) {
  g->err.clear();
  return run_group(g, [&](gpx_handle* m, int) { return gpx_predict(m, Xq, M, mean, var, mem_kind); });
}

// every rank computes the same (lml, grad) (the all-reduce inside lml_grad_impl); rank 0's is returned
int group_lml_grad(gpx_handle* g, double* lml, double* grad) {
  Group* G = g->group;
  g->err.clear();
  std::vector<double> lm(G->members.size(), 0.0), gr(G->members.size() * 34, 0.0);
  const int rc = run_group(g, [&](gpx_handle* m, int r) {
    return gpx_lml_grad(m, &lm[(size_t)r], &gr[(size_t)r * 34]);
  });
  if (rc != GPX_OK) return rc;
  const int ntheta = G->members[0]->n_ls + 2;
  *lml = lm[0];
  for (int t = 0; t < ntheta; ++t) grad[t] = gr[(size_t)t];
  return GPX_OK;
}

}  // namespace

extern "C" int gpx_debug_local_hub(int32_t P, int32_t rounds, int32_t abort_rank, int32_t abort_round,
                                   int32_t* completed) {
  if (P < 1 || P > 64 || rounds < 0 || !completed) return GPX_E_ARG;
  try {
    LocalHub hub;
    hub.init(P);
    std::vector<int> board((size_t)P, -1), fin((size_t)P, 0), bad((size_t)P, 0);
    auto body = [&](int r) {
      for (int it = 0; it < rounds; ++it) {
        if (r == abort_rank && it == abort_round) {
          hub.abort();
          return;
        }
        board[(size_t)r] = it;  // "publish" before barrier A
        if (!hub.barrier()) return;
        for (int q = 0; q < P; ++q)
          if (board[(size_t)q] != it) bad[(size_t)r] = 1;  // every peer's value of THIS round
        if (!hub.barrier()) return;  // nobody overwrites before all have read
        fin[(size_t)r] = it + 1;
      }
    };
    std::vector<std::thread> th;
    for (int r = 1; r < P; ++r) th.emplace_back(body, r);
    body(0);
    for (auto& t : th) t.join();
    int lo = rounds, any_bad = 0;
    for (int r = 0; r < P; ++r) {
      if (r != abort_rank) lo = std::min(lo, fin[(size_t)r]);
      any_bad |= bad[(size_t)r];
    }
    *completed = lo;
    return any_bad ? GPX_E_COMM : GPX_OK;
  } catch (...) {
    return GPX_E_NOMEM;
  }
}
