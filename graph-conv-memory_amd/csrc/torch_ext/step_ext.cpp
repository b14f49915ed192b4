// Host side of the per-step hot loop as a C++ autograd node.
//
// `for t: belief, m = gcm(obs[t], m)` (README.md:79-82, ray_gcm.py:200-202) is host-bound once the
// step is one kernel per direction: a Python torch.autograd.Function costs ~38 us forward and ~44 us
// backward per step in interpreter / trampoline overhead, more than the kernels take.  FusedStepFn makes
// the step's two C-ABI calls into libgcm_hip.so (gcm_dense_step_fwd / gcm_dense_step_bwd) without the
// interpreter on the path - in particular the backward runs on the autograd engine thread without taking
// the GIL.
//
// The parameter gradient of the T steps of a rollout is not summed step by step: every step node
// accumulates its per-graph slabs into ONE slab array owned by the module (slab_acc, read-modify-
// write inside the backward kernel) and returns no gradient for the parameter vector; a gate node
// between the parameter vector and the steps (gcm/_ops.py:_ParamGate) runs after all of them and
// adds the single slab sum.  The autograd engine would otherwise sum T separate [param_count]
// tensors with one tiny kernel each, after T slab-sum launches.
//
// No device code here: PyTorch is plumbing (allocation, autograd graph, stream); the product is the
// C-ABI library this file links against.
#include <cstdlib>
#include <torch/extension.h>
#include <c10/hip/HIPFunctions.h>
#include <c10/hip/HIPStream.h>
#include <c10/hip/HIPGraphsC10Utils.h>
#include <torch/csrc/autograd/python_variable.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "gcm_hip.h"

#ifdef GCM_HOST_PROF
#include <chrono>
static double g_prof[8];
static long g_prof_n;
static inline double prof_now() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
#define PROF_T(i) { const double t_ = prof_now(); g_prof[i] += t_ - prof_t; prof_t = t_; }
#else
#define PROF_T(i)
#endif

namespace {

using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

inline int64_t pad64(int64_t n) { return (n + 63) & ~int64_t(63); }

struct StepCfg {
  std::vector<gcm_selector_desc> descs;
  int act1, act2, has_bias, N, F, H1, H2;
  int cached_flags = 0;   // extra has_bias bits of the cached step only (GCM_STEP_TWO_LAUNCH: the A/B of tests / tools)
  bool col_cache = true;  // chains whose selectors write column cur take gcm_dense_rows_step_colcache (A/B switch)
  bool hops_bptt = true;  // forward-hop cached chains take gcm_dense_rows_bptt_cached_hops in their backward (A/B switch)
  bool hops_fold = true;  // ... with the hop sum folded into its products (off: ..._hops_unfolded, the kernel before; A/B switch)
  bool merge_captured = true;   // lean cached steps captured back to back become one graph node (A/B switch)
  int merge_cap = 0;            // steps per such node (tests split a run with it); 0: the library's cap
  bool absorb_head = true;      // ... and the rollout's head launch in front of step 0 is absorbed into it (A/B switch)
  bool run_mfma = true;         // ... and that node runs its layers on the fp32 matrix cores (A/B switch: the VALU form)
  int64_t P;
  bool has_distance = false;
  at::Tensor ws;   // scratch of the distance selectors
  size_t ws_bytes = 0;

  StepCfg(int64_t desc_ptr, int n_desc, int act1_, int act2_, int has_bias_, int N_, int F_,
          int H1_, int H2_)
      : act1(act1_), act2(act2_), has_bias(has_bias_), N(N_), F(F_), H1(H1_), H2(H2_) {
    descs.resize(n_desc);
    if (n_desc) std::memcpy(descs.data(), reinterpret_cast<const void*>(desc_ptr),
                            sizeof(gcm_selector_desc) * n_desc);
    for (const auto& d : descs) has_distance |= d.kind == GCM_SEL_DISTANCE;
    P = (int64_t)gcm_dense_gnn2_param_count(F, H1, H2);
  }

  void update_descs(int64_t desc_ptr, int n_desc) {   // re-read device pointers (dist_param)
    if (n_desc == (int)descs.size() && n_desc)
      std::memcpy(descs.data(), reinterpret_cast<const void*>(desc_ptr),
                  sizeof(gcm_selector_desc) * n_desc);
  }

  void* workspace(int B, const at::Tensor& like, size_t* bytes) {
    *bytes = 0;
    if (!has_distance) return nullptr;
    size_t need = 0;
    for (const auto& d : descs)
      if (d.kind == GCM_SEL_DISTANCE)
        need = std::max(need, gcm_edge_distance_workspace_bytes(d.mode, std::max(B, d.n_cur_rows), N, F));
    // (the live-row step also keeps the selector's decision row there)
    need = std::max(need, gcm_dense_rows_step_workspace_bytes(descs.data(), (int)descs.size(), B, N, F));
    if (need > ws_bytes) {
      ws = at::empty({(int64_t)need}, like.options().dtype(at::kByte));
      ws_bytes = need;
    }
    *bytes = ws_bytes;
    return ws.defined() ? ws.data_ptr() : nullptr;
  }
};

void check(int rc, const char* what) {
  TORCH_CHECK(rc == 0, what, " failed: ", gcm_status_string(rc), " (code ", rc, ")");
}

// float offsets inside the forward buffer: nodes | adj | mx | h1 | agg1 | agg2 (64-float aligned)
// ... then cur | count_out as 2*B int64 (same allocation: one caching-allocator round trip per step)
struct Layout {
  int64_t total, o_adj, o_mx, o_h1, o_agg1, o_agg2, o_idx;
  Layout(int64_t B, int64_t N, int64_t F, int64_t H1, int64_t H2, bool need_bwd) {
    const int64_t n_nodes = pad64(B * N * F), n_adj = pad64(B * N * N), n_mx = pad64(B * H2);
    const int64_t n_h1 = pad64(B * N * H1), n_agg2 = pad64(B * H1);
    o_adj = n_nodes;
    o_mx = o_adj + n_adj;
    o_h1 = o_mx + n_mx;
    o_agg1 = o_h1 + n_h1;
    o_agg2 = o_agg1 + n_nodes;
    o_idx = need_bwd ? o_agg2 + n_agg2 : o_h1;   // 64-float aligned => 8-byte aligned
    total = o_idx + pad64(4 * B);
  }
};

struct FusedStepFn : public torch::autograd::Function<FusedStepFn> {
  static variable_list forward(AutogradContext* ctx, at::Tensor obs, at::Tensor nodes_in,
                               at::Tensor packed, at::Tensor adj_in, at::Tensor count_in,
                               at::Tensor flags, int64_t cfg_handle, int64_t stream,
                               int64_t need_bwd_, at::Tensor slab_acc, int64_t is_head) {
    StepCfg* cfg = reinterpret_cast<StepCfg*>(cfg_handle);
    obs = obs.contiguous();
    nodes_in = nodes_in.contiguous();
    adj_in = adj_in.contiguous();
    const int64_t B = obs.size(0);
    const int N = cfg->N, F = cfg->F, H1 = cfg->H1, H2 = cfg->H2;
    const bool need_bwd = need_bwd_ != 0;   // decided by the caller: grad mode is off in here
    const Layout L(B, N, F, H1, H2, need_bwd);
    at::Tensor buf = at::empty({L.total}, obs.options());
    at::Tensor ibuf = buf.narrow(0, L.o_idx, 4 * B).view(at::kLong).view({2, B});
    float* base = buf.data_ptr<float>();
    int64_t* ib = ibuf.data_ptr<int64_t>();
    size_t ws_bytes = 0;
    void* ws = cfg->workspace((int)B, obs, &ws_bytes);
    const int rc = gcm_dense_step_fwd(
        obs.data_ptr<float>(), nodes_in.data_ptr<float>(), adj_in.data_ptr<float>(),
        count_in.data_ptr<int64_t>(), base, base + L.o_adj, ib, ib + B,
        cfg->descs.empty() ? nullptr : cfg->descs.data(), (int)cfg->descs.size(),
        packed.data_ptr<float>(), cfg->has_bias, cfg->act1, cfg->act2, base + L.o_mx,
        need_bwd ? base + L.o_h1 : nullptr, need_bwd ? base + L.o_agg1 : nullptr,
        need_bwd ? base + L.o_agg2 : nullptr, reinterpret_cast<uint32_t*>(flags.data_ptr()), ws,
        ws_bytes, (int)B, N, F, H1, H2, reinterpret_cast<gcm_stream_t>(stream));
    check(rc, "gcm_dense_step_fwd");
    at::Tensor nodes_out = buf.narrow(0, 0, B * N * F).view({B, N, F});
    at::Tensor adj_out = buf.narrow(0, L.o_adj, B * N * N).view({B, N, N});
    at::Tensor mx = buf.narrow(0, L.o_mx, B * H2).view({B, H2});
    at::Tensor cur = ibuf.select(0, 0), count_out = ibuf.select(0, 1);
    if (need_bwd) {
      ctx->save_for_backward({buf, count_in, packed});
      auto& sd = ctx->saved_data;
      sd["dims"] = std::vector<int64_t>{B, N, F, H1, H2, cfg->P, cfg->has_bias, cfg->act1,
                                        cfg->act2, stream, is_head};
      if (slab_acc.defined() && slab_acc.numel() == B * cfg->P) sd["slab_acc"] = slab_acc;
    }
    ctx->mark_non_differentiable({adj_out, cur, count_out});
    // undefined output gradients stay undefined (backward handles them): the engine would
    // otherwise launch one zero-fill per output and step
    ctx->set_materialize_grads(false);
    return {mx, nodes_out, adj_out, cur, count_out};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const at::Tensor &buf = saved[0], &count_in = saved[1], &packed = saved[2];
    const auto d = ctx->saved_data["dims"].toIntVector();
    const int64_t B = d[0], N = d[1], F = d[2], H1 = d[3], H2 = d[4], P = d[5];
    const int has_bias = (int)d[6], act1 = (int)d[7], act2 = (int)d[8];
    const gcm_stream_t stream = reinterpret_cast<gcm_stream_t>(d[9]);
    const Layout L(B, N, F, H1, H2, true);
    const bool is_head = d.size() > 10 && d[10] != 0;
    at::Tensor slab_acc;
    if (ctx->saved_data.count("slab_acc")) slab_acc = ctx->saved_data["slab_acc"].toTensor();
    const bool want_par = ctx->needs_input_grad(2);
    const bool deferred = want_par && slab_acc.defined();   // slabs go to the module's array
    if (!grads[0].defined() && !grads[1].defined())   // this step feeds nothing
      return {at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(),
              at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
    at::Tensor g_mx = grads[0].defined() ? grads[0].contiguous() : at::zeros({B, H2}, buf.options());
    at::Tensor g_no = grads[1].defined() ? grads[1].contiguous() : at::Tensor();
    // outputs (+ slab scratch when the sum happens here) in one allocation:
    // g_nodes_in | g_obs | g_params | slabs
    const int64_t n_nodes = pad64(B * N * F), n_obs = pad64(B * F), n_p = pad64(P);
    at::Tensor out = at::empty({n_nodes + n_obs + (deferred ? 0 : n_p + B * P)}, buf.options());
    float* ob = out.data_ptr<float>();
    const float* base = buf.data_ptr<float>();
    const int64_t* ib = reinterpret_cast<const int64_t*>(base + L.o_idx);
    if (deferred) {
      const int rc = gcm_dense_step_bwd_slabs(
          g_mx.data_ptr<float>(), g_no.defined() ? g_no.data_ptr<float>() : nullptr, base,
          base + L.o_adj, ib, count_in.data_ptr<int64_t>(), packed.data_ptr<float>(), has_bias, act1,
          act2, base + L.o_mx, base + L.o_h1, base + L.o_agg1, base + L.o_agg2, ob, ob + n_nodes,
          slab_acc.data_ptr<float>(), /*accumulate=*/1, (int)B, (int)N, (int)F, (int)H1, (int)H2,
          stream);
      check(rc, "gcm_dense_step_bwd_slabs");
    } else {
      const int rc = gcm_dense_step_bwd(
          g_mx.data_ptr<float>(), g_no.defined() ? g_no.data_ptr<float>() : nullptr, base,
          base + L.o_adj, ib, count_in.data_ptr<int64_t>(), packed.data_ptr<float>(), has_bias, act1,
          act2, base + L.o_mx, base + L.o_h1, base + L.o_agg1, base + L.o_agg2, ob, ob + n_nodes,
          ob + n_nodes + n_obs, ob + n_nodes + n_obs + n_p, sizeof(float) * (size_t)(B * P), (int)B,
          (int)N, (int)F, (int)H1, (int)H2, stream);
      check(rc, "gcm_dense_step_bwd");
    }
    at::Tensor g_obs, g_nodes_in, g_params;
    if (ctx->needs_input_grad(0)) g_obs = out.narrow(0, n_nodes, B * F).view({B, F});
    if (ctx->needs_input_grad(1)) g_nodes_in = out.narrow(0, 0, B * N * F).view({B, N, F});
    if (want_par) {
      // deferred: the gate adds the slab sum; the first step of a chain hands it a defined (zero)
      // gradient so that the gate is certain to run
      if (!deferred) g_params = out.narrow(0, n_nodes + n_obs, P);
      else if (is_head) g_params = at::zeros({P}, buf.options());
    }
    return {g_obs, g_nodes_in, g_params, at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(),
            at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
  }
};

std::vector<at::Tensor> fused_step(const at::Tensor& obs, const at::Tensor& nodes_in,
                                   const at::Tensor& packed, const at::Tensor& adj_in,
                                   const at::Tensor& count_in, const at::Tensor& flags,
                                   int64_t cfg_handle, int64_t stream,
                                   const c10::optional<at::Tensor>& slab_acc, bool is_head) {
  TORCH_CHECK(cfg_handle != 0, "fused_step: no step configuration");
  TORCH_CHECK(obs.is_cuda() && nodes_in.is_cuda() && packed.is_cuda() && adj_in.is_cuda() &&
                  count_in.is_cuda() && flags.is_cuda(),
              "fused_step: every tensor must live on a HIP device (no CPU fallback)");
  TORCH_CHECK(obs.scalar_type() == at::kFloat && nodes_in.scalar_type() == at::kFloat &&
              adj_in.scalar_type() == at::kFloat && packed.scalar_type() == at::kFloat &&
              count_in.scalar_type() == at::kLong && packed.is_contiguous() &&
              count_in.is_contiguous());
  const bool need_bwd = at::GradMode::is_enabled() &&
                        (obs.requires_grad() || nodes_in.requires_grad() || packed.requires_grad());
  return FusedStepFn::apply(obs, nodes_in, packed, adj_in, count_in, flags, cfg_handle, stream,
                            (int64_t)need_bwd,
                            slab_acc.has_value() ? *slab_acc : at::empty({0}, obs.options()),
                            (int64_t)is_head);
}


// ---------------------------------------------------------------------------------------------
// The live-row step (rows_step.hip / rows_bptt.hip): one kernel per forward step, donated or
// functional state, and NO kernel and NO autograd node per backward step.  With no gradient flowing
// into observations or nodes, step t's adjoint depends on g_mx[t] and step t's own record only, so
// every step of a chain of hidden states hangs its belief tensor on ONE node (RowsChainNode: forward
// output k = step k's mx).  The engine delivers all g_mx at once and the node hands every recorded
// graph-step to one time-parallel launch (gcm_dense_rows_bptt).  Round 2 had one node per step plus a
// gate node: ~8 us of engine time per step, more than the kernel takes.
// ---------------------------------------------------------------------------------------------
// A contiguous tensor over part of `base`'s storage WITHOUT a view relation (no narrow/view dispatches,
// no view bookkeeping: ~0.1 us instead of ~1.5 us per pair on the per-step host path).  It has its own
// version counter.  offset in elements of `dtype`.
static at::Tensor alias_of(const at::Tensor& base, int64_t offset, at::IntArrayRef sizes, caffe2::TypeMeta dtype) {
  auto impl = c10::make_intrusive<c10::TensorImpl>(c10::Storage(base.storage()), base.key_set(), dtype);
  // (offset: elements of `dtype` behind base's own first element - base may itself be an alias into a larger block)
  offset += base.storage_offset() * (int64_t)base.dtype().itemsize() / (int64_t)dtype.itemsize();
  impl->set_storage_offset(offset);
  impl->set_sizes_contiguous(sizes);
  return at::Tensor(std::move(impl));
}

struct RowsChainNode : public torch::autograd::Node {
  struct Rec {
    at::Tensor buf;             // the step's record (gcm_dense_rows_layout); starts with mx
    c10::VariableVersion vc;    // version counter of the belief tensor handed to the caller (it aliases
    uint32_t version;           // the head of the record) and its value when recorded
    int out_mx = -1;            // which of this node's outputs the belief tensor is
    int out_nodes = -1;         // dx: ... and the returned node matrix
    int edge_x = -1;            // dx: the next edge that leads to this step's observation (-1: no gradient)
    bool cached = false;        // a cached step (rows_cached.hip): the live rows are in the chain's caches
    int cur = -1;               // ... and, hop_rows set, the row it wrote: known on the host.  hop_rows: ANY cached step of a
    bool hop_rows = false;      // chain without a distance selector (lean or not: cur_host = the chain's step count in both)
  };
  at::Tensor cH, cA, cX;        // the caches of the chain's cached steps
  bool many_rows = false;       // a DenseEdge selector: every row <= cur is live (GCM_BPTT_MANY_ROWS)
  bool hops_bptt = true;        // StepCfg::hops_bptt when the chain was armed
  bool hops_fold = true;        // StepCfg::hops_fold when the chain was armed
  std::vector<gcm_selector_desc> descs;   // ... and the selectors their live rows follow from (dx of cached steps)
  std::vector<Rec> recs;   // the recorded steps, in chain order
  at::Tensor packed;       // the packed parameter vector, detached (the kernel re-reads the weights)
  int N = 0, F = 0, H1 = 0, H2 = 0, has_bias = 0, act1 = 0, act2 = 0;
  int64_t P = 0;           // floats the backward kernel writes (GNN gradient | d c1 with the deg term)
  bool executed = false, released = false;
  // dx: the chain also differentiates w.r.t. its observations (and the node matrix it started from) - all of
  // it in this ONE node, time-parallel (gcm_dense_rows_bptt_dx_all).  An observation's producer is younger
  // than this node, and Node::add_next_edge refuses new edges once a node has parents (it could no longer
  // keep parent.topological_nr > child.topological_nr for them).  The invariant is what matters, not the
  // bookkeeping: this node starts with a topological number far above any ordinary graph's (2^40), appends
  // an observation's edge directly when the producer's number is below its own - which also proves the
  // producer does not depend on this chain's outputs (an ancestor's number would be larger) - and reports
  // failure otherwise (a policy that feeds belief t-1 into observation t: one node per step, DxStepNode).
  bool dx = false, want_gn0 = false;
  int edge_gn0 = -1;
  int64_t B = 0;
  at::Tensor count0;       // num_nodes entering the first step
  void start_dx() {
    dx = true;
    if (topological_nr_ < (1ull << 40)) topological_nr_ = 1ull << 40;
  }
  bool can_take(const at::Tensor& obs) const {
    if (!obs.requires_grad()) return true;
    const auto e = torch::autograd::impl::gradient_edge(obs);
    if (!e.function) return true;
    return e.function->topological_nr() < topological_nr_ || recs.empty();
  }
  int take_x_edge(const at::Tensor& obs) {   // -> index of the new next edge, -1: none needed
    if (!obs.requires_grad()) return -1;
    auto e = torch::autograd::impl::gradient_edge(obs);
    if (!e.function) return -1;
    const uint64_t p = e.function->topological_nr();
    if (p >= topological_nr_) {
      TORCH_CHECK(recs.empty(), "rows chain: observation depends on this chain's outputs");
      topological_nr_ = p + (1ull << 32);   // first step, no parents yet: sit above the producer (stacked memories)
    }
    next_edges().push_back(std::move(e));
    return (int)next_edges().size() - 1;
  }
  void apply_dx(variable_list& grads, variable_list& out, gcm_stream_t stream) {
    const int K = (int)recs.size();
    at::Tensor gx = at::zeros({K, B, F}, packed.options());
    at::Tensor gn0 = want_gn0 ? at::zeros({B, N, F}, packed.options()) : at::Tensor();
    // belief gradients with common element strides (an expanded one is read with stride 0; mixed strides:
    // contiguous copies); node-matrix gradients contiguous
    std::vector<at::Tensor> gms(K), gns(K);
    int64_t sb = 0, sh = 0;
    bool have = false, mixed = false;
    for (int k = 0; k < K; ++k) {
      const Rec& r = recs[k];
      at::Tensor g = r.out_mx >= 0 ? grads[r.out_mx] : at::Tensor();
      if (g.defined()) {
        if (g.scalar_type() != at::kFloat) g = g.to(at::kFloat);
        if (!have) { sb = g.stride(0); sh = g.stride(1); have = true; }
        mixed = mixed || g.stride(0) != sb || g.stride(1) != sh;
        gms[k] = g;
      }
      at::Tensor n = r.out_nodes >= 0 ? grads[r.out_nodes] : at::Tensor();
      if (n.defined()) gns[k] = n.to(at::kFloat).contiguous();
    }
    if (mixed) {
      for (auto& g : gms)
        if (g.defined()) g = g.contiguous();
      sb = H2;
      sh = 1;
    }
    std::vector<const float*> sv(K, nullptr), gm(K, nullptr), gn(K, nullptr);
    for (int k = 0; k < K; ++k) {
      sv[k] = recs[k].buf.data_ptr<float>();
      if (gms[k].defined()) gm[k] = gms[k].data_ptr<float>();
      if (gns[k].defined()) gn[k] = gns[k].data_ptr<float>();
    }
    constexpr int CHUNK = 64;   // steps per launch (gcm_dense_rows_bptt_dx_all), of one kind (cached | not)
    for (int k0 = 0, n = 0; k0 < K; k0 += n) {
      const bool kind = recs[k0].cached;
      n = 1;
      while (n < CHUNK && k0 + n < K && recs[k0 + n].cached == kind) ++n;
      bool any = false;
      for (int k = k0; k < k0 + n; ++k) any = any || gm[k] || gn[k];
      if (!any) continue;
      if (kind) {
        check(gcm_dense_rows_bptt_dx_all_cached(sv.data() + k0, gm.data() + k0, (long)sb, (long)sh, n, k0,
                                                packed.data_ptr<float>(), has_bias, act1, act2,
                                                descs.empty() ? nullptr : descs.data(), (int)descs.size(),
                                                cH.data_ptr<float>(), gx.data_ptr<float>(), (int)B, N, F, H1, H2, stream),
              "gcm_dense_rows_bptt_dx_all_cached");
        continue;
      }
      check(gcm_dense_rows_bptt_dx_all(sv.data() + k0, gm.data() + k0, (long)sb, (long)sh, gn.data() + k0, n, k0,
                                       packed.data_ptr<float>(), has_bias, act1, act2, count0.data_ptr<int64_t>(),
                                       gx.data_ptr<float>(), gn0.defined() ? gn0.data_ptr<float>() : nullptr, (int)B,
                                       N, F, H1, H2, stream),
            "gcm_dense_rows_bptt_dx_all");
    }
    for (int k = 0; k < K; ++k)
      if (recs[k].edge_x >= 0 && task_should_compute_output(recs[k].edge_x)) out[recs[k].edge_x] = gx.select(0, k);
    if (edge_gn0 >= 0 && gn0.defined() && task_should_compute_output(edge_gn0)) out[edge_gn0] = gn0;
  }
  variable_list apply(variable_list&& grads) override {
    executed = true;
    TORCH_CHECK(!released, "Trying to backward through the live-row steps of a DenseGCM chain a second "
                           "time (their records were freed); pass retain_graph=True to the first call");
    variable_list out(num_outputs());
    TORCH_CHECK(grads.size() == num_inputs(), "rows chain: ", grads.size(), " gradients for ", num_inputs(),
                " outputs of ", recs.size(), " recorded steps");
    // groups of steps with equal batch size and gradient strides (an expanded gradient, as mean()
    // produces, is read with stride 0 - no .contiguous() copies), in first-seen order
    struct Group {
      int64_t B, sb, sh;
      bool cached;
      std::vector<const float*> sv, gm;
      std::vector<uint8_t> cur;
    };
    // the GEMM-form backward (gcm_dense_rows_bptt_cached_hops): only while EVERY step of the chain is a cached step with
    // a host-known row - a chain that left that case mid-way keeps the kernel that reads the records' live lists
    // (GCM_BPTT_PER_ITEM=1, the A/B of the record walk's two kernels, asks for the record walk: it wins)
    static const bool want_walk = std::getenv("GCM_BPTT_PER_ITEM") && std::getenv("GCM_BPTT_PER_ITEM")[0] == '1';
    bool hop_chain = hops_bptt && !want_walk && !recs.empty() && cH.defined();
    int rows_written = 0;
    for (const Rec& r : recs) {
      hop_chain = hop_chain && r.cached && r.hop_rows && r.cur >= 0 && r.cur < 128;
      rows_written = std::max(rows_written, r.cur + 1);
    }
    std::vector<Group> groups;
    std::vector<at::Tensor> keep;
    for (size_t k = 0; k < recs.size(); ++k) {
      const Rec& r = recs[k];
      if (!grads[r.out_mx].defined()) continue;
      TORCH_CHECK(r.vc.current_version() == r.version,
                  "one of the variables needed for gradient computation has been modified by an inplace "
                  "operation: the belief states returned by DenseGCM step ", k, " of this chain (version ",
                  r.vc.current_version(), ", expected ", r.version,
                  ") are part of the record its backward reads");
      at::Tensor g = grads[r.out_mx];
      if (g.scalar_type() != at::kFloat) {
        g = g.to(at::kFloat);
        keep.push_back(g);
      }
      const int64_t B = g.size(0), sb = g.stride(0), sh = g.stride(1);
      Group* grp = nullptr;
      for (auto& c : groups)
        if (c.B == B && c.sb == sb && c.sh == sh && c.cached == r.cached) grp = &c;
      if (!grp) {
        groups.push_back({B, sb, sh, r.cached, {}, {}, {}});
        grp = &groups.back();
      }
      grp->sv.push_back(r.buf.data_ptr<float>());
      grp->gm.push_back(g.data_ptr<float>());
      grp->cur.push_back((uint8_t)(r.cur & 0xff));
    }
    const gcm_stream_t stream =
        reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(packed.get_device()).stream());
    if (dx) apply_dx(grads, out, stream);
    if (groups.empty()) return out;
    at::Tensor prev;
    for (auto& c : groups) {
      const int n = (int)c.sv.size();
      const bool hops = c.cached && hop_chain && c.B == cH.size(0);
      // (the GEMM form writes one slab per graph)
      const size_t ws_bytes = std::max(gcm_dense_rows_bptt_workspace_bytes(n, (int)c.B, F, H1, H2),
                                       hops ? sizeof(float) * (size_t)P * (size_t)c.B : (size_t)0);
      at::Tensor ws = at::empty({(int64_t)ws_bytes}, packed.options().dtype(at::kByte));
      // the kernel writes the first P floats; constant sections behind them get a zero gradient
      at::Tensor res = packed.numel() > P ? at::zeros({packed.numel()}, packed.options())
                                          : at::empty({P}, packed.options());
      // (GCM_BPTT_PER_ITEM=1: the per-item backward kernel where the per-graph form exists - the A/B; a per-call flag of the
      //  C ABI, read from the environment by this host module once)
      static const int per_item = (std::getenv("GCM_BPTT_PER_ITEM") && std::getenv("GCM_BPTT_PER_ITEM")[0] == '1')
                                      ? GCM_STEP_FOUR_WAVES : 0;
      int hops_rc = GCM_EUNSUPPORTED;
      if (hops)
        hops_rc = (hops_fold ? gcm_dense_rows_bptt_cached_hops : gcm_dense_rows_bptt_cached_hops_unfolded)(
                                                  c.sv.data(), c.gm.data(), n, (long)c.sb, (long)c.sh,
                                                  packed.data_ptr<float>(), has_bias, act1, act2, cX.data_ptr<float>(),
                                                  cH.data_ptr<float>(), cA.data_ptr<float>(), c.cur.data(),
                                                  descs.empty() ? nullptr : descs.data(), (int)descs.size(), rows_written,
                                                  prev.defined() ? prev.data_ptr<float>() : nullptr,
                                                  res.data_ptr<float>(), ws.data_ptr(), ws_bytes, (int)c.B, N, F, H1, H2,
                                                  stream);
      if (hops_rc != GCM_EUNSUPPORTED)   // (unsupported: a case the GEMM form has no kernel for - the record walk below)
        check(hops_rc, "gcm_dense_rows_bptt_cached_hops");
      else if (c.cached)
        check(gcm_dense_rows_bptt_cached(c.sv.data(), c.gm.data(), n, (long)c.sb, (long)c.sh, packed.data_ptr<float>(),
                                         has_bias | per_item, act1, act2, cX.data_ptr<float>(), cH.data_ptr<float>(),
                                         cA.data_ptr<float>(), prev.defined() ? prev.data_ptr<float>() : nullptr,
                                         res.data_ptr<float>(), ws.data_ptr(), ws_bytes, (int)c.B, N, F, H1, H2, stream),
              "gcm_dense_rows_bptt_cached");
      else
      check(gcm_dense_rows_bptt(c.sv.data(), c.gm.data(), n, (long)c.sb, (long)c.sh,
                                packed.data_ptr<float>(), has_bias | (many_rows ? GCM_BPTT_MANY_ROWS : 0), act1, act2,
                                prev.defined() ? prev.data_ptr<float>() : nullptr, res.data_ptr<float>(),
                                ws.data_ptr(), ws_bytes, (int)c.B, N, F, H1, H2, stream),
            "gcm_dense_rows_bptt");
      prev = res;
    }
    out[0] = prev;
    return out;
  }
  void release_variables() override {
    recs.clear();
    released = true;
  }
  std::string name() const override { return "GcmRowsChain"; }
};

// ---------------------------------------------------------------------------------------------
// Live-row steps whose observations (or the node matrix the chain started from) need a gradient.
// An observation's producer is younger than the head of the chain, and autograd edges only reach older
// nodes - so no single node can return all of them: here every step IS a node (DxStepNode: inputs its
// observation, the previous step, the gate), but a light one.  The engine runs them last step first (each
// depends on its successor); a step's launch (gcm_dense_rows_bptt_dx_step, one wave per graph) adds its few
// rows of dL/dx into the accumulators of the nodes they belong to (gx: one [B,F] slot per step), so by the
// time step k runs, slot k is complete and is what it returns.  The parameter gradient accumulates in the
// chain's slab array; the gate (created at the head: inputs the packed vector and the head's node matrix)
// runs after every step and sums it once.
// ---------------------------------------------------------------------------------------------
struct DxChain {
  at::Tensor packed;    // detached
  at::Tensor count0;    // num_nodes entering the first step
  at::Tensor gx, gn0;   // accumulators of the running backward pass
  at::Tensor zero_p;
  // (record, g_mx) of the steps of the running pass: their parameter gradient is ONE time-parallel launch
  // by the gate (gcm_dense_rows_bptt; the dx sections of a record sit behind the ones it reads)
  std::vector<at::Tensor> p_bufs, p_gmx;
  int N = 0, F = 0, H1 = 0, H2 = 0, has_bias = 0, act1 = 0, act2 = 0;
  int64_t P = 0, T = 0, B = 0;
  int pass = -2;        // graph task the accumulators belong to
  bool want_gn0 = false, gave_defined = false, executed = false;

  void begin_pass_if_new() {
    const int id = torch::autograd::get_current_graph_task_id();
    if (id == pass && gx.defined() && gx.size(0) == T) return;
    pass = id;
    gx = at::zeros({T, B, F}, packed.options());
    gn0 = want_gn0 ? at::zeros({B, N, F}, packed.options()) : at::Tensor();
    p_bufs.clear();      // (a pass whose gate never ran, e.g. autograd.grad w.r.t. the observations only)
    p_gmx.clear();
    gave_defined = false;
  }
};

struct DxGateNode : public torch::autograd::Node {
  std::shared_ptr<DxChain> ch;
  variable_list apply(variable_list&& grads) override {
    variable_list out(2);
    ch->executed = true;
    if (ch->pass != torch::autograd::get_current_graph_task_id()) return out;   // no step ran
    const gcm_stream_t stream =
        reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(ch->packed.get_device()).stream());
    // groups of steps with equal gradient strides (an expanded gradient is read with stride 0)
    at::Tensor prev;
    std::vector<char> done(ch->p_bufs.size(), 0);
    for (size_t i = 0; i < ch->p_bufs.size(); ++i) {
      if (done[i]) continue;
      const int64_t sb = ch->p_gmx[i].stride(0), sh = ch->p_gmx[i].stride(1);
      std::vector<const float*> sv, gm;
      for (size_t j = i; j < ch->p_bufs.size(); ++j)
        if (!done[j] && ch->p_gmx[j].stride(0) == sb && ch->p_gmx[j].stride(1) == sh) {
          sv.push_back(ch->p_bufs[j].data_ptr<float>());
          gm.push_back(ch->p_gmx[j].data_ptr<float>());
          done[j] = 1;
        }
      const int n = (int)sv.size();
      const size_t ws_bytes = gcm_dense_rows_bptt_workspace_bytes(n, (int)ch->B, ch->F, ch->H1, ch->H2);
      at::Tensor ws = at::empty({(int64_t)ws_bytes}, ch->packed.options().dtype(at::kByte));
      at::Tensor res = at::empty({ch->P}, ch->packed.options());
      check(gcm_dense_rows_bptt(sv.data(), gm.data(), n, (long)sb, (long)sh, ch->packed.data_ptr<float>(),
                                ch->has_bias, ch->act1, ch->act2, prev.defined() ? prev.data_ptr<float>() : nullptr,
                                res.data_ptr<float>(), ws.data_ptr(), ws_bytes, (int)ch->B, ch->N, ch->F, ch->H1,
                                ch->H2, stream),
            "gcm_dense_rows_bptt");
      prev = res;
    }
    out[0] = prev;
    if (ch->gn0.defined() && task_should_compute_output(1)) out[1] = ch->gn0;
    ch->p_bufs.clear();
    ch->p_gmx.clear();
    ch->gx = at::Tensor();
    ch->gn0 = at::Tensor();
    ch->pass = -2;
    return out;
  }
  std::string name() const override { return "GcmRowsDxGate"; }
};

struct DxStepNode : public torch::autograd::Node {
  std::shared_ptr<DxChain> ch;
  at::Tensor buf;
  c10::VariableVersion vc;
  uint32_t version = 0;
  int64_t k = 0;

  variable_list apply(variable_list&& grads) override {   // grads: belief, (successor), returned node matrix
    variable_list out(3);
    TORCH_CHECK(buf.defined(), "Trying to backward through a live-row step of a DenseGCM chain a second time (its "
                               "record was freed); pass retain_graph=True to the first call");
    ch->executed = true;
    ch->begin_pass_if_new();
    at::Tensor g = grads[0], gn = grads[2];
    if (g.defined()) {
      TORCH_CHECK(vc.current_version() == version,
                  "one of the variables needed for gradient computation has been modified by an inplace "
                  "operation: the belief states returned by DenseGCM step ", k, " of this chain");
      if (g.scalar_type() != at::kFloat) g = g.to(at::kFloat);
    }
    if (gn.defined()) gn = gn.to(at::kFloat).contiguous();
    const gcm_stream_t stream =
        reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(ch->packed.get_device()).stream());
    check(gcm_dense_rows_bptt_dx_step(
              buf.data_ptr<float>(), g.defined() ? g.data_ptr<float>() : nullptr, g.defined() ? (long)g.stride(0) : 0,
              g.defined() ? (long)g.stride(1) : 0, gn.defined() ? gn.data_ptr<float>() : nullptr,
              ch->packed.data_ptr<float>(), ch->has_bias, ch->act1, ch->act2, ch->count0.data_ptr<int64_t>(),
              ch->gx.data_ptr<float>(), ch->gn0.defined() ? ch->gn0.data_ptr<float>() : nullptr, (int)k, (int)ch->B,
              ch->N, ch->F, ch->H1, ch->H2, stream),
          "gcm_dense_rows_bptt_dx_step");
    if (g.defined()) {
      ch->p_bufs.push_back(buf);
      ch->p_gmx.push_back(g);
    }
    if (task_should_compute_output(0)) out[0] = ch->gx.select(0, k);
    if (!ch->gave_defined) {   // one defined gradient per pass, so that the gate is certain to run
      if (!ch->zero_p.defined()) ch->zero_p = at::zeros({ch->packed.numel()}, ch->packed.options());
      out[2] = ch->zero_p;
      ch->gave_defined = true;
    }
    return out;
  }
  void release_variables() override { buf.reset(); }
  std::string name() const override { return "GcmRowsDxStep"; }
};

// ---------------------------------------------------------------------------------------------------------------
struct RecordPool {
  // The records of the cached steps are small (the belief, the live list, a few vectors): sixteen of them come out of ONE
  // allocation (the caching allocator's at::empty was 1.0 us of a 5.7 us step, tools/hosttime.py; an alias into the block
  // is 0.2).  A block is released when the last of its records is - a caller that keeps one belief keeps fifteen small
  // neighbours alive.  One block per stream: the allocator knows a block by the stream it was allocated on.
  // ... and one block per stream CAPTURE: memory allocated while a HIP graph is captured belongs to that graph's private
  // pool (a block from outside it may be freed and reused while the graph still writes there on replay; a block of
  // another capture dies with that graph).
  at::Tensor rec_block;
  int64_t rec_size = 0, rec_used = 0;
  void* rec_stream = nullptr;
  unsigned long long rec_capture = 0;
  int capturing = -1;   // what the last take() saw of its stream: 1 being captured, 0 not, -1 it did not look
  static constexpr int64_t REC_PER_BLOCK = 16;
  at::Tensor take(int64_t floats, const at::Tensor& like, int dev) {
    const int64_t n = pad64(floats);
    capturing = -1;
    if (n * (int64_t)sizeof(float) > (1 << 20)) return at::empty({n}, like.options());   // (large records: their own allocation)
    hipStream_t st = c10::hip::getCurrentHIPStream(dev).stream();
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    unsigned long long cid = 0;
    if (hipStreamGetCaptureInfo(st, &cs, &cid) != hipSuccess || cs != hipStreamCaptureStatusActive) cid = 0;
    capturing = cid != 0 ? 1 : 0;
    if (!rec_block.defined() || rec_size != n || rec_used == REC_PER_BLOCK || rec_stream != (void*)st || rec_capture != cid) {
      rec_block = at::empty({REC_PER_BLOCK * n}, like.options());
      rec_size = n;
      rec_used = 0;
      rec_stream = (void*)st;
      rec_capture = cid;
    }
    return alias_of(rec_block, (rec_used++) * n, {n}, rec_block.dtype());
  }
};

// The per-step host path of `belief, m = gcm(obs, m)` on the live-row kernels.  One instance per
// (DenseGCM module, step configuration).  `run` is the checked entry (Python validated the hidden
// state and built the packed parameter vector); `step` is what DenseGCM.__call__ tries first: when
// the hidden state is the very tuple of tensors the previous call returned, the observation has the
// same shape, the parameters are the same objects at the same versions and grad mode has not
// changed, everything `run` needs is known to hold and the step is ONE call from Python: two
// allocations, one launch, one output registered on the chain node.  Anything else returns None and
// Python takes the checked path.
struct RowsFast {
  StepCfg* cfg = nullptr;
  at::Tensor packed, flags;
  bool donate = false, grad_mode = false, armed = false;
  bool dx_mode = false;   // the armed chain differentiates w.r.t. observations / nodes:
  int dx_kind = 0;        //   1 in its one chain node, time-parallel (RowsChainNode::dx); 2 one node per step (DxStepNode)
  bool dx_steps_only = false;   // an observation depended on this module's own outputs once: kind 2 from then on
  // cached steps (rows_cached.hip): the armed chain started from the empty graphs of hidden = None on a donated
  // state, its selectors only write row cur, it is linear and has made fewer than N steps
  bool cache_ok = false;
  // ... and past N steps, in the steady state (every graph full, every step drops its oldest node), while the
  // selectors are forward temporal hops with N > 2 max(hop): gcm_dense_rows_step_cached_roll - the caches as rings,
  // the band adjacency untouched, the node matrix rolled in place
  bool roll_ok = false;
  // ... or while the only selector is EuclideanEdge in its one-launch form (no `learned` divisor, local batch):
  // gcm_edge_distance_step_ring - the roll in the same launch, the live rows re-evaluated from the chain's bit image of
  // the adjacency (abits, kept by the cached steps)
  bool ring_ok = false;
  // ... or (round 6) the chain's selectors also write COLUMN cur - DenseEdge, "backward" / "both" hops - on a donated
  // or functional state from empty graphs: gcm_dense_rows_step_colcache (rank-1 updates of the chain's float64 agg1 cache, one MFMA
  // product of the live rows), the general live-row record; past N steps its ring form
  bool col_ok = false;
  int64_t cached_steps = 0, chain_steps = 0, rolled_steps = 0, col_steps = 0;
  at::Tensor cH, cA, cX, wimg, abits;
  // the weight image the fused head launch (pack_params_head) made beside a packed vector, and that vector: taken by
  // the chain's first cached step iff it is armed with that very tensor
  at::Tensor head_img, head_img_of;
  at::Tensor kA, kR;   // the column-write chain's caches: agg1 [B,N,F] in float64, root [B,N,H1]
  at::Tensor rH, rA, rX;   // the ring caches of the steady-state steps (copies: the first N records keep reading cH / cA / cX)
  std::shared_ptr<DxChain> dxc;
  std::shared_ptr<DxGateNode> dx_gate;
  std::shared_ptr<DxStepNode> dx_last;
  std::shared_ptr<RowsChainNode> node;
  std::vector<pybind11::object> hook_dicts;    // the module's and torch's global hook dicts: all must be empty
  std::vector<pybind11::object> dicts, keys;   // module._parameters dicts and the names read from them
  std::vector<pybind11::object> objs;          // the Parameter objects (or None) the packed vector was built from
  std::vector<uint32_t> vers;
  at::Tensor l_nodes, l_adj, l_weights, l_count;   // the hidden state returned last
  // ... and its version counters right after the launch: the kernels write through raw pointers, so only a caller's
  // in-place edit (e.g. zeroing the graphs of finished episodes in a donated state) moves them - a cached step, which
  // reads its per-chain caches and the host's step count instead of the state, must then not run
  uint32_t lv_nodes = 0, lv_adj = 0, lv_count = 0;
  int64_t xB = -1, xF = -1, n_steps = 0;

  void note_versions() {
    lv_nodes = l_nodes._version();
    lv_adj = l_adj._version();
    lv_count = l_count._version();
  }
  bool state_untouched() const {
    return l_nodes.defined() && l_nodes._version() == lv_nodes && l_adj._version() == lv_adj &&
           l_count._version() == lv_count;
  }
  int dev = -1;
  // the chain's run object (gcm_hip_run.h): inside a stream capture, cached lean steps that follow one another directly
  // are appended to ONE graph node.  Reset whenever the chain is re-armed or a step comes through the checked entry.
  void* mrun = nullptr;
  int mrun_cap = 0, mrun_absorb = -1, mrun_mfma = -1;

  RowsFast(const std::vector<std::pair<pybind11::object, pybind11::object>>& specs,
           const std::vector<pybind11::object>& hooks)
      : hook_dicts(hooks) {
    for (const auto& s : specs) {
      dicts.push_back(s.first);
      keys.push_back(s.second);
    }
  }
  RowsFast(const RowsFast&) = delete;
  RowsFast& operator=(const RowsFast&) = delete;
  ~RowsFast() {
    if (mrun) gcm_rows_run_destroy(mrun);
  }
  bool last_cached_eager = true;   // the last cached step ran outside a capture: merge_stats() is then {0, 0}
  // nullptr: the switch is off, or the record pool has just seen that the stream is not being captured - the step is
  // then gcm_dense_rows_step_cached_ws exactly, without a second look at the stream (a capture query is ~1 us of host
  // time, a fifth of an eager step)
  void* merge_run() {
    last_cached_eager = rec_pool.capturing == 0;
    if (!cfg->merge_captured || rec_pool.capturing == 0) return nullptr;
    if (!mrun) mrun = gcm_rows_run_create();
    const int cap = cfg->merge_cap > 0 ? std::min(cfg->merge_cap, gcm_rows_run_steps_cap()) : gcm_rows_run_steps_cap();
    if (mrun && cap != mrun_cap) {
      gcm_rows_run_set_cap(mrun, cap);
      mrun_cap = cap;
    }
    set_absorb(cfg->absorb_head);
    if (mrun && (int)cfg->run_mfma != mrun_mfma) {
      gcm_rows_run_set_mfma(mrun, cfg->run_mfma ? 1 : 0);
      mrun_mfma = (int)cfg->run_mfma;
    }
    return mrun;
  }
  void set_absorb(bool on) {
    if (mrun && (int)on != mrun_absorb) {
      gcm_rows_run_set_absorb(mrun, on ? 1 : 0);
      mrun_absorb = (int)on;
    }
  }
  // the run object for the head launch of forward(x, None) (pack_params_head): the chain this head starts is armed
  // right behind it.  nullptr with the switches off: the head is then gcm_dense_rows_head_fused exactly
  void* head_run(bool on) {
    if (!on) {
      set_absorb(false);
      return nullptr;
    }
    if (!mrun) mrun = gcm_rows_run_create();
    set_absorb(true);
    return mrun;
  }
  std::pair<int, int> merge_stats() const {
    int out[2] = {0, 0};
    if (mrun && !last_cached_eager) gcm_rows_run_stats(mrun, out);
    return {out[0], out[1]};
  }
  bool run_mfma() const { return mrun ? gcm_rows_run_mfma(mrun) != 0 : (cfg ? cfg->run_mfma : true); }
  int head_absorbed() const { return mrun && !last_cached_eager ? gcm_rows_run_absorbed(mrun) : 0; }

  bool hooks_registered() const {   // torch.nn.Module.__call__ has work to do: take the long way
    for (const auto& d : hook_dicts)
      if (PyObject_Size(d.ptr()) != 0) return true;
    return false;
  }

  bool params_current() const {
    for (size_t i = 0; i < dicts.size(); ++i) {
      PyObject* o = PyDict_GetItem(dicts[i].ptr(), keys[i].ptr());   // borrowed
      if (o != objs[i].ptr()) return false;
      if (o && THPVariable_Check(o) && THPVariable_Unpack(o)._version() != vers[i]) return false;
    }
    return true;
  }

  // A donated state is advanced in place, which autograd does not allow for a tensor that carries a gradient:
  // with the one-node form of the observation gradient (kind 1) the records alone serve the backward, so the
  // state may still be donated - the returned node matrix is then a plain tensor (no gradient through it);
  // not when the chain starts from a node matrix that itself needs a gradient, nor with one node per step.
  static bool want_donate(bool donate_, int dx_, const at::Tensor& head_nodes) {
    return donate_ && (dx_ == 0 || (dx_ == 1 && !(head_nodes.defined() && head_nodes.requires_grad())));
  }
  void arm(const at::Tensor& packed_, const at::Tensor& flags_, int64_t cfg_handle, bool donate_, int dx_ = 0,
           const at::Tensor& head_nodes = at::Tensor(), const at::Tensor& head_count = at::Tensor(),
           bool fresh = false) {
    cfg = reinterpret_cast<StepCfg*>(cfg_handle);
    packed = packed_;
    flags = flags_;
    donate = want_donate(donate_, dx_, head_nodes);
    dx_mode = false;
    dx_kind = 0;
    grad_mode = at::GradMode::is_enabled();
    dev = packed.get_device();
    objs.clear();
    vers.clear();
    for (size_t i = 0; i < dicts.size(); ++i) {
      PyObject* o = PyDict_GetItem(dicts[i].ptr(), keys[i].ptr());
      objs.push_back(o ? pybind11::reinterpret_borrow<pybind11::object>(o) : pybind11::object());
      vers.push_back(o && THPVariable_Check(o) ? THPVariable_Unpack(o)._version() : 0);
    }
    node.reset();
    dxc.reset();
    dx_gate.reset();
    dx_last.reset();
    if (grad_mode && packed.requires_grad() && dx_)
      TORCH_CHECK(gcm_dense_rows_dx_supported(cfg->N, cfg->F, cfg->H1, cfg->H2) &&
                      !(cfg->has_bias & (GCM_GNN_HAS_DEG_TERM | GCM_GNN_HAS_PE_TABLE)),
                  "rows step: this configuration has no observation-gradient form");
    if (grad_mode && packed.requires_grad() && dx_ == 2) {
      dx_mode = true;
      dx_kind = 2;
      dxc = std::make_shared<DxChain>();
      dxc->packed = packed.detach();
      dxc->count0 = head_count;
      dxc->N = cfg->N; dxc->F = cfg->F; dxc->H1 = cfg->H1; dxc->H2 = cfg->H2;
      dxc->has_bias = cfg->has_bias; dxc->act1 = cfg->act1; dxc->act2 = cfg->act2;
      dxc->P = (int64_t)gcm_dense_gnn2_param_count(cfg->F, cfg->H1, cfg->H2);
      dxc->B = head_count.size(0);
      dxc->want_gn0 = head_nodes.defined() && head_nodes.requires_grad();
      dx_gate = std::shared_ptr<DxGateNode>(new DxGateNode(), torch::autograd::deleteNode);
      dx_gate->ch = dxc;
      dx_gate->set_next_edges(torch::autograd::collect_next_edges(packed));
      dx_gate->add_next_edge(dxc->want_gn0 ? torch::autograd::impl::gradient_edge(head_nodes)
                                           : torch::autograd::Edge());
      dx_gate->add_input_metadata(packed);
    } else if (grad_mode && packed.requires_grad()) {
      node = std::shared_ptr<RowsChainNode>(new RowsChainNode(), torch::autograd::deleteNode);
      node->packed = packed.detach();
      node->N = cfg->N; node->F = cfg->F; node->H1 = cfg->H1; node->H2 = cfg->H2;
      node->has_bias = cfg->has_bias; node->act1 = cfg->act1; node->act2 = cfg->act2;
      node->P = (int64_t)gcm_dense_gnn2_param_count(cfg->F, cfg->H1, cfg->H2) +
                ((cfg->has_bias & GCM_GNN_HAS_DEG_TERM) ? cfg->H1 : 0);
      TORCH_CHECK(packed.numel() >= node->P, "rows step: packed parameter vector too short");
      for (const auto& d : cfg->descs) node->many_rows = node->many_rows || d.kind == GCM_SEL_DENSE;
      node->hops_bptt = cfg->hops_bptt;
      node->hops_fold = cfg->hops_fold;
      node->set_next_edges(torch::autograd::collect_next_edges(packed));
      if (dx_ == 1) {
        dx_mode = true;
        dx_kind = 1;
        node->count0 = head_count;
        node->B = head_count.size(0);
        node->want_gn0 = head_nodes.defined() && head_nodes.requires_grad();
        if (node->want_gn0) {
          node->add_next_edge(torch::autograd::impl::gradient_edge(head_nodes));
          node->edge_gn0 = (int)node->num_outputs() - 1;
        }
        node->start_dx();
      }
    }
    chain_steps = cached_steps = rolled_steps = col_steps = 0;
    cH = cA = cX = rH = rA = rX = abits = kA = kR = at::Tensor();
    if (mrun) gcm_rows_run_reset(mrun);
    // (a distance selector's decisions reach the cached step as a row: no hop table to rebuild the live rows from
    //  in the observation-gradient launch - those chains stay on the general kernel)
    cache_ok = fresh && donate && dx_kind != 2 && !(cfg->has_distance && dx_kind != 0) &&
               gcm_dense_rows_cached_supported_ws(cfg->descs.empty() ? nullptr : cfg->descs.data(),
                                                  (int)cfg->descs.size(), cfg->has_bias, cfg->N, cfg->F, cfg->H1,
                                                  cfg->H2) != 0;
    // (observation gradients follow the rows of the node matrix back to their steps by position: such chains hand
    //  the rolling regime to the kernel that records the rows' positions)
    roll_ok = cache_ok && dx_kind == 0 &&
              gcm_dense_rows_cached_roll_supported(cfg->descs.empty() ? nullptr : cfg->descs.data(),
                                                   (int)cfg->descs.size(), cfg->has_bias, cfg->N, cfg->F, cfg->H1,
                                                   cfg->H2) != 0;
    ring_ok = cache_ok && dx_kind == 0 && cfg->descs.size() == 1 && cfg->descs[0].kind == GCM_SEL_DISTANCE &&
              cfg->descs[0].mode == GCM_DIST_EUCLID_CROSSBATCH && !cfg->descs[0].bidirectional &&
              cfg->descs[0].dist_param == nullptr && cfg->descs[0].cur_rows == nullptr && !(cfg->has_bias & ~3) &&
              !(cfg->cached_flags & GCM_STEP_TWO_LAUNCH);
    // (donated or functional state: the functional form writes the new state from extra workgroups of its launch)
    col_ok = !cache_ok && fresh && dx_kind == 0 && !cfg->has_distance && cfg->col_cache &&
             gcm_dense_rows_colcache_supported(cfg->descs.empty() ? nullptr : cfg->descs.data(), (int)cfg->descs.size(),
                                               cfg->has_bias, cfg->N, cfg->F, cfg->H1, cfg->H2) != 0;
    armed = true;
  }

  // a step of a chain whose selectors write column cur too (see col_ok): one launch, the general live-row record
  at::Tensor launch_colcache(const at::Tensor& obs, const at::Tensor& nodes_in, const at::Tensor& adj_in,
                             const at::Tensor& weights, const at::Tensor& count_in) {
    const int64_t B = obs.size(0);
    const int N = cfg->N, F = cfg->F, H1 = cfg->H1, H2 = cfg->H2;
    const bool need_bwd = node != nullptr;
    if (cached_steps == 0) {   // (uninitialised: a row is read only after the step that wrote it)
      kA = at::empty({B, N, F}, obs.options().dtype(at::kDouble));
      kR = at::empty({B, N, H1}, obs.options());
    }
    size_t lay[8];
    check(gcm_dense_rows_layout((int)B, N, F, H1, H2, lay), "gcm_dense_rows_layout");
    at::Tensor buf = at::empty({need_bwd ? (int64_t)lay[0] : pad64(B * H2)}, obs.options());
    const gcm_stream_t stream = reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(dev).stream());
    at::Tensor nodes_out = nodes_in, adj_out = adj_in, count_out = count_in;
    if (donate) {
      check(gcm_dense_rows_step_colcache(obs.data_ptr<float>(), nodes_in.data_ptr<float>(), adj_in.data_ptr<float>(),
                                         count_in.data_ptr<int64_t>(), cfg->descs.data(), (int)cfg->descs.size(),
                                         packed.data_ptr<float>(), cfg->has_bias, cfg->act1, cfg->act2,
                                         kA.data_ptr<double>(), kR.data_ptr<float>(), buf.data_ptr<float>(),
                                         need_bwd ? 1 : 0, (int)cached_steps,
                                         reinterpret_cast<uint32_t*>(flags.data_ptr()), (int)B, N, F, H1, H2, stream),
            "gcm_dense_rows_step_colcache");
    } else {   // functional state: one allocation for the new nodes | adj | count, as the general step makes it
      const int64_t n_nodes = pad64(B * N * F), n_adj = pad64(B * (int64_t)N * N);
      at::Tensor st = at::empty({n_nodes + n_adj + pad64(2 * B)}, obs.options());
      nodes_out = alias_of(st, 0, {B, N, F}, st.dtype());
      adj_out = alias_of(st, n_nodes, {B, N, N}, st.dtype());
      count_out = alias_of(st, (n_nodes + n_adj) / 2, {B}, caffe2::TypeMeta::Make<int64_t>());
      check(gcm_dense_rows_step_colcache_functional(
                obs.data_ptr<float>(), nodes_in.data_ptr<float>(), adj_in.data_ptr<float>(),
                count_in.data_ptr<int64_t>(), nodes_out.data_ptr<float>(), adj_out.data_ptr<float>(),
                count_out.data_ptr<int64_t>(), cfg->descs.data(), (int)cfg->descs.size(), packed.data_ptr<float>(),
                cfg->has_bias, cfg->act1, cfg->act2, kA.data_ptr<double>(), kR.data_ptr<float>(), buf.data_ptr<float>(),
                need_bwd ? 1 : 0, (int)cached_steps, reinterpret_cast<uint32_t*>(flags.data_ptr()), (int)B, N, F, H1,
                H2, stream),
            "gcm_dense_rows_step_colcache_functional");
    }
    at::Tensor mx = alias_of(buf, 0, {B, H2}, buf.dtype());
    if (need_bwd) {
      const c10::VariableVersion& vc = mx.unsafeGetTensorImpl()->version_counter();
      RowsChainNode::Rec r{buf, vc, vc.current_version()};   // (cached = false: its rows travel in the record)
      r.out_mx = (int)node->num_inputs();
      torch::autograd::create_gradient_edge(mx, node);
      node->recs.push_back(std::move(r));
    }
    l_nodes = nodes_out;
    l_adj = adj_out;
    l_weights = weights;
    l_count = count_out;
    note_versions();
    xB = B;
    xF = obs.size(1);
    ++n_steps;
    ++chain_steps;
    ++cached_steps;
    ++col_steps;
    return mx;
  }

  // the steady-state step of an EuclideanEdge chain (see ring_ok): one launch, the general live-row record
  at::Tensor launch_ring(const at::Tensor& obs, const at::Tensor& nodes_in, const at::Tensor& adj_in,
                         const at::Tensor& weights, const at::Tensor& count_in) {
    const int64_t B = obs.size(0);
    const int N = cfg->N, F = cfg->F, H1 = cfg->H1, H2 = cfg->H2;
    const bool need_bwd = node != nullptr;
    size_t lay[8];
    check(gcm_dense_rows_layout((int)B, N, F, H1, H2, lay), "gcm_dense_rows_layout");
    at::Tensor buf = at::empty({need_bwd ? (int64_t)lay[0] : pad64(B * H2)}, obs.options());
    const gcm_stream_t stream = reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(dev).stream());
    check(gcm_edge_distance_step_ring(obs.data_ptr<float>(), nodes_in.data_ptr<float>(), adj_in.data_ptr<float>(),
                                      count_in.data_ptr<int64_t>(), cfg->descs[0].max_distance, packed.data_ptr<float>(),
                                      wimg.data_ptr<float>(), cfg->act1, cfg->act2,
                                      reinterpret_cast<uint32_t*>(abits.data_ptr()), buf.data_ptr<float>(), lay,
                                      need_bwd ? 1 : 0, reinterpret_cast<uint32_t*>(flags.data_ptr()), (int)B, N, F, H1, H2,
                                      stream),
          "gcm_edge_distance_step_ring");
    at::Tensor mx = alias_of(buf, 0, {B, H2}, buf.dtype());
    if (need_bwd) {
      const c10::VariableVersion& vc = mx.unsafeGetTensorImpl()->version_counter();
      RowsChainNode::Rec r{buf, vc, vc.current_version()};   // (cached = false: its rows travel in the record)
      r.out_mx = (int)node->num_inputs();
      torch::autograd::create_gradient_edge(mx, node);
      node->recs.push_back(std::move(r));
    }
    l_nodes = nodes_in;
    l_adj = adj_in;
    l_weights = weights;
    l_count = count_in;
    note_versions();
    xB = B;
    xF = obs.size(1);
    ++n_steps;
    ++chain_steps;
    ++cached_steps;
    ++rolled_steps;
    return mx;
  }

  // a cached step in the steady state (see roll_ok): the general live-row record, the state's node matrix rolled in
  // place by the same launch, adjacency and count as they are
  RecordPool rec_pool;
  at::Tensor take_record(int64_t floats, const at::Tensor& like) { return rec_pool.take(floats, like, dev); }

  at::Tensor launch_cached_roll(const at::Tensor& obs, const at::Tensor& nodes_in, const at::Tensor& adj_in,
                                const at::Tensor& weights, const at::Tensor& count_in) {
    const int64_t B = obs.size(0);
    const int N = cfg->N, F = cfg->F, H1 = cfg->H1, H2 = cfg->H2;
    const bool need_bwd = node != nullptr;
    if (rolled_steps == 0) {
      // A ring slot is overwritten N steps later, but the records of the first N steps read their rows from the
      // caches when the backward runs: the rings start as copies (once per chain; no backward, no copy)
      if (need_bwd) { rH = cH.clone(); rA = cA.clone(); rX = cX.clone(); }
      else { rH = cH; rA = cA; rX = cX; }
    }
    size_t lay[8];
    check(gcm_dense_rows_layout((int)B, N, F, H1, H2, lay), "gcm_dense_rows_layout");
    at::Tensor buf = take_record(need_bwd ? (int64_t)lay[0] : B * H2, obs);
    const gcm_stream_t stream = reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(dev).stream());
    check(gcm_dense_rows_step_cached_roll(obs.data_ptr<float>(), nodes_in.data_ptr<float>(),
                                          cfg->descs.empty() ? nullptr : cfg->descs.data(), (int)cfg->descs.size(),
                                          packed.data_ptr<float>(), wimg.data_ptr<float>(), cfg->has_bias, cfg->act1,
                                          cfg->act2, rH.data_ptr<float>(), rA.data_ptr<float>(), rX.data_ptr<float>(),
                                          buf.data_ptr<float>(), need_bwd ? 1 : 0, (int)cached_steps,
                                          reinterpret_cast<uint32_t*>(flags.data_ptr()), (int)B, N, F, H1, H2, stream),
          "gcm_dense_rows_step_cached_roll");
    at::Tensor mx = alias_of(buf, 0, {B, H2}, buf.dtype());
    if (need_bwd) {
      const c10::VariableVersion& vc = mx.unsafeGetTensorImpl()->version_counter();
      RowsChainNode::Rec r{buf, vc, vc.current_version()};   // (cached = false: its rows travel in the record)
      r.out_mx = (int)node->num_inputs();
      torch::autograd::create_gradient_edge(mx, node);
      node->recs.push_back(std::move(r));
    }
    l_nodes = nodes_in;
    l_adj = adj_in;
    l_weights = weights;
    l_count = count_in;
    note_versions();
    xB = B;
    xF = obs.size(1);
    ++n_steps;
    ++chain_steps;
    ++cached_steps;
    ++rolled_steps;
    return mx;
  }

  // a cached step (see cache_ok): one small launch, the record without a rows section
  at::Tensor launch_cached(const at::Tensor& obs, const at::Tensor& nodes_in, const at::Tensor& adj_in,
                           const at::Tensor& weights, const at::Tensor& count_in) {
    const int64_t B = obs.size(0);
    const int N = cfg->N, F = cfg->F, H1 = cfg->H1, H2 = cfg->H2;
    const bool need_bwd = node != nullptr;
    if (cached_steps == 0) {
      // (no zero fill: forward and backward read a row only behind a select on "written before" - three 4 MB fill
      //  launches per chain were 2 % of a graph-replayed cfg2 rollout)
      cH = at::empty({B, N, H1}, obs.options());
      cA = at::empty({B, N, F}, obs.options());
      cX = at::empty({B, N, F}, obs.options());
      if (node) { node->cH = cH; node->cA = cA; node->cX = cX; node->descs = cfg->descs; }
      // the weights lane-major, once per chain (the parameters are fixed inside one): the image that came with this
      // very packed vector out of the head's one launch, or a launch of its own
      if (head_img.defined() && head_img_of.unsafeGetTensorImpl() == packed.unsafeGetTensorImpl() &&
          head_img.numel() == (int64_t)gcm_dense_rows_cached_weight_image_floats()) {
        wimg = head_img;
      } else {
        wimg = at::empty({(int64_t)gcm_dense_rows_cached_weight_image_floats()}, obs.options());
        check(gcm_dense_rows_cached_weight_image(packed.data_ptr<float>(), wimg.data_ptr<float>(), F, H1, H2,
                                                 reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(dev).stream())),
              "gcm_dense_rows_cached_weight_image");
      }
      head_img = head_img_of = at::Tensor();
    }
#ifdef GCM_HOST_PROF
    double prof_t = prof_now();
#endif
    size_t lay[5];
    check(gcm_dense_rows_cached_layout((int)B, N, F, H1, H2, lay), "gcm_dense_rows_cached_layout");
    at::Tensor buf = take_record(need_bwd ? (int64_t)lay[0] : B * H2, obs);
    PROF_T(1)
    const gcm_stream_t stream = reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(dev).stream());
    size_t ws_bytes = 0;
    void* ws = cfg->workspace((int)B, obs, &ws_bytes);   // (a distance selector's scratch and decision row)
    if (ring_ok && cached_steps == 0) {
      ring_ok = gcm_edge_distance_step_cached_supported((int)B, (int)B, N, F, H1, H2) &&
                gcm_edge_distance_step_ring_supported((int)B, N, F, H1, H2);
      if (ring_ok) abits = at::zeros({B, (int64_t)N, 4}, obs.options().dtype(at::kInt));
    }
    if (ring_ok) {   // EuclideanEdge alone, one launch: called directly, so that it also keeps the chain's bit image
      check(gcm_edge_distance_step_cached(obs.data_ptr<float>(), nodes_in.data_ptr<float>(), adj_in.data_ptr<float>(),
                                          count_in.data_ptr<int64_t>(), cfg->descs[0].max_distance, nullptr, nullptr, 0,
                                          packed.data_ptr<float>(), wimg.data_ptr<float>(), cfg->act1, cfg->act2,
                                          cH.data_ptr<float>(), cA.data_ptr<float>(), cX.data_ptr<float>(),
                                          buf.data_ptr<float>(), lay, need_bwd ? 1 : 0, (int)cached_steps,
                                          reinterpret_cast<uint32_t*>(abits.data_ptr()),
                                          reinterpret_cast<uint32_t*>(flags.data_ptr()), (int)B, N, F, H1, H2, stream),
            "gcm_edge_distance_step_cached");
    } else   // (with the chain's run object: captured back to back, lean steps share one graph node - gcm_hip_run.h)
    check(gcm_dense_rows_step_cached_run(merge_run(), obs.data_ptr<float>(), nodes_in.data_ptr<float>(),
                                         adj_in.data_ptr<float>(), count_in.data_ptr<int64_t>(),
                                         cfg->descs.empty() ? nullptr : cfg->descs.data(), (int)cfg->descs.size(),
                                         packed.data_ptr<float>(), wimg.data_ptr<float>(),
                                         cfg->has_bias | cfg->cached_flags, cfg->act1, cfg->act2, cH.data_ptr<float>(),
                                         cA.data_ptr<float>(), cX.data_ptr<float>(), buf.data_ptr<float>(),
                                         need_bwd ? 1 : 0, (int)cached_steps,
                                         reinterpret_cast<uint32_t*>(flags.data_ptr()), ws, ws_bytes, (int)B, N, F, H1,
                                         H2, stream),
          "gcm_dense_rows_step_cached_run");
    PROF_T(2)
    at::Tensor mx = alias_of(buf, 0, {B, H2}, buf.dtype());
    PROF_T(3)
    if (need_bwd) {
      const c10::VariableVersion& vc = mx.unsafeGetTensorImpl()->version_counter();
      RowsChainNode::Rec r{buf, vc, vc.current_version()};
      r.cached = true;
      r.cur = (int)cached_steps;
      r.hop_rows = !cfg->has_distance;
      if (dx_kind == 1) r.edge_x = node->take_x_edge(obs);
      r.out_mx = (int)node->num_inputs();
      torch::autograd::create_gradient_edge(mx, node);
      node->recs.push_back(std::move(r));
    }
    PROF_T(4)
    l_nodes = nodes_in;
    l_adj = adj_in;
    l_weights = weights;
    l_count = count_in;
    xB = B;
    xF = obs.size(1);
    note_versions();
    ++n_steps;
    ++chain_steps;
    ++cached_steps;
    return mx;
  }

  // one step; inputs validated by the caller.  -> mx; the new state lands in l_*
  at::Tensor launch(const at::Tensor& obs, const at::Tensor& nodes_in, const at::Tensor& adj_in,
                    const at::Tensor& weights, const at::Tensor& count_in) {
    const int64_t B = obs.size(0);
    const int N = cfg->N, F = cfg->F, H1 = cfg->H1, H2 = cfg->H2;
    if (cache_ok && cached_steps == chain_steps && (cached_steps == 0 || (cH.size(0) == B && state_untouched()))) {
      if (cached_steps < N) return launch_cached(obs, nodes_in, adj_in, weights, count_in);
      // (t_abs as an int, ring slots from it: a chain of 2^31 steps ends the cached run)
      if (roll_ok && cached_steps < (int64_t)0x7fffffff) return launch_cached_roll(obs, nodes_in, adj_in, weights, count_in);
      if (ring_ok && abits.defined()) return launch_ring(obs, nodes_in, adj_in, weights, count_in);
    }
    // (below N steps and - the ring form - past them: every step then drops the oldest node)
    if (col_ok && cached_steps == chain_steps && cached_steps < (int64_t)0x7fffffff &&
        (cached_steps == 0 || (kA.size(0) == B && state_untouched())))
      return launch_colcache(obs, nodes_in, adj_in, weights, count_in);
    cache_ok = col_ok = false;
    ++chain_steps;
    const bool need_bwd = node != nullptr || dxc != nullptr;
    size_t lay[8];
    if (dx_mode) check(gcm_dense_rows_layout_dx((int)B, N, F, H1, H2, lay), "gcm_dense_rows_layout_dx");
    else check(gcm_dense_rows_layout((int)B, N, F, H1, H2, lay), "gcm_dense_rows_layout");
    at::Tensor buf = at::empty({need_bwd ? (int64_t)lay[0] : pad64(B * H2)}, obs.options());
    at::Tensor nodes_out, adj_out, count_out;
    if (donate) {
      nodes_out = nodes_in;
      adj_out = adj_in;
      count_out = count_in;
    } else {
      const int64_t n_nodes = pad64(B * N * F), n_adj = pad64(B * (int64_t)N * N);
      at::Tensor st = at::empty({n_nodes + n_adj + pad64(2 * B)}, obs.options());
      nodes_out = alias_of(st, 0, {B, N, F}, st.dtype());
      adj_out = alias_of(st, n_nodes, {B, N, N}, st.dtype());
      count_out = alias_of(st, (n_nodes + n_adj) / 2, {B}, caffe2::TypeMeta::Make<int64_t>());
    }
    size_t ws_bytes = 0;
    void* ws = cfg->workspace((int)B, obs, &ws_bytes);
    const gcm_stream_t stream = reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(dev).stream());
    check(gcm_dense_rows_step_fwd_ws(
              obs.data_ptr<float>(), nodes_in.data_ptr<float>(), adj_in.data_ptr<float>(),
              count_in.data_ptr<int64_t>(), nodes_out.data_ptr<float>(), adj_out.data_ptr<float>(),
              count_out.data_ptr<int64_t>(), nullptr, cfg->descs.empty() ? nullptr : cfg->descs.data(),
              (int)cfg->descs.size(), packed.data_ptr<float>(), cfg->has_bias | (dx_mode ? GCM_GNN_RECORD_DX : 0),
              cfg->act1, cfg->act2, buf.data_ptr<float>(), need_bwd ? buf.data_ptr<float>() : nullptr,
              reinterpret_cast<uint32_t*>(flags.data_ptr()), ws, ws_bytes, (int)B, N, F, H1, H2, stream),
          "gcm_dense_rows_step_fwd_ws");
    at::Tensor mx = alias_of(buf, 0, {B, H2}, buf.dtype());   // the record starts with the belief states
    if (dxc) {   // one light node per step: inputs its observation, its predecessor, the gate
      auto sn = std::shared_ptr<DxStepNode>(new DxStepNode(), torch::autograd::deleteNode);
      sn->ch = dxc;
      sn->buf = buf;
      sn->vc = mx.unsafeGetTensorImpl()->version_counter();
      sn->version = sn->vc.current_version();
      sn->k = dxc->T++;
      sn->add_next_edge(obs.requires_grad() ? torch::autograd::impl::gradient_edge(obs) : torch::autograd::Edge());
      sn->add_next_edge(dx_last ? torch::autograd::Edge(dx_last, 1) : torch::autograd::Edge());
      sn->add_next_edge(torch::autograd::Edge(dx_gate, 0));
      torch::autograd::create_gradient_edge(mx, sn);                      // output 0
      sn->add_input_metadata(torch::autograd::Node::undefined_input{});   // output 1: what the successor hangs on
      torch::autograd::create_gradient_edge(nodes_out, sn);               // output 2
      dx_last = sn;
    } else if (need_bwd) {
      const c10::VariableVersion& vc = mx.unsafeGetTensorImpl()->version_counter();
      RowsChainNode::Rec r{buf, vc, vc.current_version()};
      if (dx_kind == 1) r.edge_x = node->take_x_edge(obs);   // (before the record joins: the first step may re-seat the node)
      r.out_mx = (int)node->num_inputs();
      torch::autograd::create_gradient_edge(mx, node);
      if (dx_kind == 1 && !donate) {
        r.out_nodes = (int)node->num_inputs();
        torch::autograd::create_gradient_edge(nodes_out, node);
      }
      node->recs.push_back(std::move(r));
    }
    l_nodes = nodes_out;
    l_adj = adj_out;
    l_weights = weights;
    l_count = count_out;
    note_versions();
    xB = B;
    xF = obs.size(1);
    ++n_steps;
    return mx;
  }

  bool continues(const at::Tensor& nodes, const at::Tensor& adj, const at::Tensor& weights,
                 const at::Tensor& count) const {
    return armed && nodes.unsafeGetTensorImpl() == l_nodes.unsafeGetTensorImpl() &&
           adj.unsafeGetTensorImpl() == l_adj.unsafeGetTensorImpl() &&
           weights.unsafeGetTensorImpl() == l_weights.unsafeGetTensorImpl() &&
           count.unsafeGetTensorImpl() == l_count.unsafeGetTensorImpl();
  }

  // the checked entry -> (mx, nodes, adj, num_nodes)
  pybind11::tuple run(const at::Tensor& obs, const at::Tensor& nodes_in, const at::Tensor& adj_in,
                      const at::Tensor& weights, const at::Tensor& count_in, const at::Tensor& packed_,
                      const at::Tensor& flags_, int64_t cfg_handle, bool donate_, int need_dx, bool fresh) {
    StepCfg* c = reinterpret_cast<StepCfg*>(cfg_handle);
    TORCH_CHECK(c != nullptr, "rows_step: no step configuration");
    TORCH_CHECK(obs.is_cuda() && nodes_in.is_cuda() && adj_in.is_cuda() && count_in.is_cuda() &&
                    packed_.is_cuda() && flags_.is_cuda(),
                "rows_step: every tensor must live on a HIP device (no CPU fallback)");
    TORCH_CHECK(obs.scalar_type() == at::kFloat && nodes_in.scalar_type() == at::kFloat &&
                adj_in.scalar_type() == at::kFloat && packed_.scalar_type() == at::kFloat &&
                count_in.scalar_type() == at::kLong && obs.is_contiguous() && nodes_in.is_contiguous() &&
                adj_in.is_contiguous() && packed_.is_contiguous() && count_in.is_contiguous());
    const int64_t B = obs.size(0);
    TORCH_CHECK(obs.dim() == 2 && nodes_in.dim() == 3 && adj_in.dim() == 3 && nodes_in.size(0) == B &&
                    nodes_in.size(1) == c->N && nodes_in.size(2) == c->F && adj_in.size(0) == B &&
                    adj_in.size(1) == c->N && adj_in.size(2) == c->N && count_in.dim() == 1 &&
                    count_in.size(0) == B && obs.size(1) == c->F,
                "rows_step: hidden state and observation shapes disagree");
    TORCH_CHECK(obs.get_device() == c10::hip::current_device() && nodes_in.get_device() == obs.get_device() &&
                    packed_.get_device() == obs.get_device(),
                "rows_step: tensors must live on the current device");
    if (!(at::GradMode::is_enabled() && packed_.requires_grad())) need_dx = 0;
    if (need_dx == 1 && dx_steps_only) need_dx = 2;
    // a chain that differentiates w.r.t. its inputs holds ONE chain of hidden states: a state that is not
    // the one returned last starts a new node (whose input 1 is that state's node matrix)
    bool new_chain = (need_dx || dx_mode) && !(dx_mode && dx_kind == need_dx && continues(nodes_in, adj_in, weights, count_in));
    if (!new_chain && dx_kind == 1 && node && !node->can_take(obs)) {
      // this observation was computed from the chain's own outputs: a single node would sit on a cycle
      dx_steps_only = true;
      need_dx = 2;
      new_chain = true;
    }
    if (!armed || c != cfg || packed_.unsafeGetTensorImpl() != packed.unsafeGetTensorImpl() ||
        flags_.unsafeGetTensorImpl() != flags.unsafeGetTensorImpl() || want_donate(donate_, need_dx, nodes_in) != donate ||
        grad_mode != at::GradMode::is_enabled() || (node && node->executed) || (dxc && dxc->executed) || new_chain ||
        (fresh && need_dx == 0))   // (a rollout from empty graphs: its own chain node - it may own caches; donated or -
                                   //  the column-write cached steps - functional state)
      arm(packed_, flags_, cfg_handle, donate_, need_dx, nodes_in, count_in, fresh);
    else if ((cache_ok || col_ok) && !continues(nodes_in, adj_in, weights, count_in))
      cache_ok = col_ok = false;
    if (mrun) gcm_rows_run_reset(mrun);   // (only the unchecked entry, which knows the chain continues, appends to a node)
    at::Tensor mx = launch(obs, nodes_in, adj_in, weights, count_in);
    return pybind11::make_tuple(mx, l_nodes, l_adj, l_count, donate);
  }

  // the unchecked entry: (mx, hidden) or None
  pybind11::object step(pybind11::handle x, pybind11::handle hidden) {
#ifdef GCM_HOST_PROF
    double prof_t = prof_now();
    ++g_prof_n;
#endif
    if (!armed || !PyTuple_Check(hidden.ptr()) || PyTuple_GET_SIZE(hidden.ptr()) != 4 ||
        !THPVariable_Check(x.ptr()))
      return pybind11::none();
    PyObject* h = hidden.ptr();
    PyObject *pn = PyTuple_GET_ITEM(h, 0), *pa = PyTuple_GET_ITEM(h, 1), *pw = PyTuple_GET_ITEM(h, 2),
             *pc = PyTuple_GET_ITEM(h, 3);
    if (!THPVariable_Check(pn) || !THPVariable_Check(pa) || !THPVariable_Check(pw) || !THPVariable_Check(pc))
      return pybind11::none();
    if (!continues(THPVariable_Unpack(pn), THPVariable_Unpack(pa), THPVariable_Unpack(pw),
                   THPVariable_Unpack(pc)))
      return pybind11::none();
    const at::Tensor& xt = THPVariable_Unpack(x.ptr());
    const bool grad = at::GradMode::is_enabled();
    if (grad != grad_mode || (node && node->executed) || (dxc && dxc->executed) || xt.dim() != 2 || xt.size(0) != xB ||
        xt.size(1) != xF || xt.scalar_type() != at::kFloat || !xt.is_cuda() || xt.get_device() != dev ||
        c10::hip::current_device() != dev || (grad && xt.requires_grad() && !dx_mode) || !params_current() ||
        hooks_registered() || (dx_kind == 1 && !node->can_take(xt)) || (dx_mode && !state_untouched()))
      return pybind11::none();
    at::Tensor obs = xt.is_contiguous() ? xt : xt.contiguous();
    PROF_T(0)
    at::Tensor mx = launch(obs, l_nodes, l_adj, l_weights, l_count);
#ifdef GCM_HOST_PROF
    prof_t = prof_now();
#endif
    pybind11::object pmx = pybind11::reinterpret_steal<pybind11::object>(THPVariable_Wrap(mx));
    if (donate) {
      pybind11::tuple r_ = pybind11::make_tuple(pmx, pybind11::reinterpret_borrow<pybind11::object>(h));
      PROF_T(5)
      return r_;
    }
    pybind11::object hn = pybind11::reinterpret_steal<pybind11::object>(PyTuple_New(4));
    PyTuple_SET_ITEM(hn.ptr(), 0, THPVariable_Wrap(l_nodes));
    PyTuple_SET_ITEM(hn.ptr(), 1, THPVariable_Wrap(l_adj));
    Py_INCREF(pw);
    PyTuple_SET_ITEM(hn.ptr(), 2, pw);
    PyTuple_SET_ITEM(hn.ptr(), 3, THPVariable_Wrap(l_count));
    return pybind11::make_tuple(pmx, hn);
  }

  // the chain differentiates w.r.t. its observations (their gradient follows the rows of the node matrix back to the
  // steps that inserted them, by position) and the caller has written into the state this chain returned last
  bool edited_dx_state(const at::Tensor& nodes, const at::Tensor& adj, const at::Tensor& weights,
                       const at::Tensor& count) const {
    return dx_mode && continues(nodes, adj, weights, count) && !state_untouched();
  }
  int64_t pending() const { return node && !node->executed ? (int64_t)node->recs.size() : 0; }
  void forget() {   // drop the packed vector (and with it the references into its autograd graph)
    armed = false;
    node.reset();
    dxc.reset();
    dx_gate.reset();
    dx_last.reset();
    packed = at::Tensor();
    head_img = head_img_of = at::Tensor();
  }
  void set_head_image(const at::Tensor& packed_, const at::Tensor& image) {
    head_img_of = packed_;
    head_img = image;
  }
};

// ---------------------------------------------------------------------------------------------
// DenseGCM + LearnedEdge (default edge network, observations without gradient): the static
// configuration that the chain below, LearnedFast and the rollout read.
// ---------------------------------------------------------------------------------------------
struct LearnedCfg {
  int N, F, H1, H2, act1, act2, has_bias;
  double eps0, eps1, cutoff;
  int64_t P, P_total;
  LearnedCfg(int N_, int F_, int H1_, int H2_, int act1_, int act2_, int has_bias_, double e0, double e1,
             double cutoff_)
      : N(N_), F(F_), H1(H1_), H2(H2_), act1(act1_), act2(act2_), has_bias(has_bias_), eps0(e0), eps1(e1),
        cutoff(cutoff_) {
    P = (int64_t)gcm_dense_gnn2_param_count(F, H1, H2);
    P_total = P + (int64_t)gcm_learned_mlp_param_count(F);
  }
};

// ---------------------------------------------------------------------------------------------
// The steps (state advance, edge network and gumbel selection, GNN forward: csrc/learned_step.hip): every
// step of a chain of hidden states hangs its belief tensor on ONE node (as the live-row steps do) and the
// backward is time-parallel
// (gcm_learned_bptt: two passes over all recorded graph-steps, no [B,N,N] gradient chain buffer, no
// kernel and no autograd node per step).  Steps form a tree through their `parent` (the step that
// produced the hidden state they continued); every root-to-leaf path is one gcm_learned_bptt call,
// with g_mx = 0 for the steps an earlier path already accounted for (everything downstream of g_mx and
// of the adjacency gradient is linear, so shared ancestors simply receive each branch's share).
// ---------------------------------------------------------------------------------------------
struct LearnedChainNode : public torch::autograd::Node {
  struct Rec {
    at::Tensor buf;             // gcm_learned_step_layout
    c10::VariableVersion vc;    // of the belief tensor (aliases buf)
    uint32_t version;
    int parent;                 // index of the step whose hidden state this one continued, or -1
    int64_t B;
    bool cached = false;        // a cached step (gcm_learned_step_cached): buf in the compact = 2 layout
  };
  std::vector<Rec> recs;
  at::Tensor packed;            // detached
  LearnedCfg* cfg = nullptr;
  bool executed = false, released = false;
  bool compact = false;         // the steps ran on a donated state: their buffers hold row cur of the adjacency only
  at::Tensor cH, cA, cX;        // the caches of the chain's cached steps (h1, agg1, node matrix of every node)
  at::Tensor cU;                // ... and the first-layer product of the edge network on every node (exact shapes only)

  variable_list apply(variable_list&& grads) override {
    executed = true;
    variable_list out(1);
    TORCH_CHECK(!released, "Trying to backward through the LearnedEdge steps of a DenseGCM chain a second time "
                           "(their records were freed); pass retain_graph=True to the first call");
    TORCH_CHECK(grads.size() == recs.size(), "learned chain: ", grads.size(), " gradients for ", recs.size(),
                " recorded steps");
    const int n = (int)recs.size();
    std::vector<char> has_child(n, 0), done(n, 0);
    bool any = false;
    for (int i = 0; i < n; ++i) {
      if (recs[i].parent >= 0) has_child[recs[i].parent] = 1;
      any |= grads[i].defined();
    }
    if (!any) return out;
    const int N = cfg->N, F = cfg->F, H1 = cfg->H1, H2 = cfg->H2;
    const gcm_stream_t stream =
        reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(packed.get_device()).stream());
    at::Tensor prev;
    std::vector<at::Tensor> keep;
    for (int leaf = 0; leaf < n; ++leaf) {
      if (has_child[leaf]) continue;
      std::vector<int> path;
      for (int i = leaf; i >= 0; i = recs[i].parent) path.push_back(i);
      std::reverse(path.begin(), path.end());
      // gradients of the steps this path owns, with common strides
      std::vector<at::Tensor> g(path.size());
      bool same = true, first = true, owned_any = false;
      int64_t sb = 0, sh = 0;
      for (size_t t = 0; t < path.size(); ++t) {
        const int i = path[t];
        if (done[i] || !grads[i].defined()) continue;
        const Rec& r = recs[i];
        TORCH_CHECK(r.vc.current_version() == r.version,
                    "one of the variables needed for gradient computation has been modified by an inplace "
                    "operation: the belief states returned by DenseGCM (LearnedEdge) step ", i);
        g[t] = grads[i].scalar_type() == at::kFloat ? grads[i] : grads[i].to(at::kFloat);
        if (first) { sb = g[t].stride(0); sh = g[t].stride(1); first = false; }
        same &= g[t].stride(0) == sb && g[t].stride(1) == sh;
        owned_any = true;
      }
      for (int i : path) done[i] = 1;
      if (!owned_any) continue;
      if (!same) {
        for (auto& t : g)
          if (t.defined()) t = t.contiguous();
        sb = H2; sh = 1;
      }
      std::vector<const float*> sv(path.size()), gm(path.size());
      for (size_t t = 0; t < path.size(); ++t) {
        sv[t] = recs[path[t]].buf.data_ptr<float>();
        gm[t] = g[t].defined() ? g[t].data_ptr<float>() : nullptr;
        if (g[t].defined()) keep.push_back(g[t]);
      }
      const int T = (int)path.size(), B = (int)recs[path[0]].B;
      int n_cached = 0;   // (cached steps are a prefix of every path: they end at the first fork / overflow risk)
      while (n_cached < T && recs[path[n_cached]].cached) ++n_cached;
      for (int t = n_cached; t < T; ++t) TORCH_CHECK(!recs[path[t]].cached, "learned chain: cached step behind a full one");
      const size_t ws_bytes = gcm_learned_bptt_workspace_bytes(T, B, N, F, H1, H2);
      at::Tensor ws = at::empty({(int64_t)ws_bytes}, packed.options().dtype(at::kByte));
      at::Tensor res = at::empty({cfg->P_total}, packed.options());
      // (GCM_BPTT_MLP_BLOCKS=1: pass B2 on the 32-row-block kernel at every shape - the A/B of tools/ab_cfg5.sh)
      static const int b2_blocks = (std::getenv("GCM_BPTT_MLP_BLOCKS") && std::getenv("GCM_BPTT_MLP_BLOCKS")[0] == '1')
                                       ? GCM_BPTT_MLP_BLOCKS : 0;
      check(gcm_learned_bptt_cached(sv.data(), gm.data(), T, n_cached, (compact ? 2 : 3) | b2_blocks,
                                    n_cached ? cX.data_ptr<float>() : nullptr,
                                    n_cached ? cH.data_ptr<float>() : nullptr,
                                    n_cached ? cA.data_ptr<float>() : nullptr,
                                    n_cached && cU.defined() ? cU.data_ptr<float>() : nullptr, (long)sb, (long)sh,
                                    packed.data_ptr<float>(), cfg->act1, cfg->act2, (float)cfg->eps0,
                                    (float)cfg->eps1, compact ? 1 : 0,
                                    prev.defined() ? prev.data_ptr<float>() : nullptr, res.data_ptr<float>(),
                                    ws.data_ptr(), ws_bytes, B, N, F, H1, H2, stream),
            "gcm_learned_bptt_cached");
      prev = res;
    }
    out[0] = prev;
    return out;
  }
  void release_variables() override {
    recs.clear();
    released = true;
  }
  std::string name() const override { return "GcmLearnedChain"; }
};

struct LearnedChain {   // one per packed parameter vector
  std::shared_ptr<LearnedChainNode> node;
  LearnedCfg* cfg;
  at::Tensor packed;
  bool donate;
  LearnedChain(int64_t cfg_handle, const at::Tensor& packed_, bool donate_)
      : cfg(reinterpret_cast<LearnedCfg*>(cfg_handle)), packed(packed_), donate(donate_) {
    TORCH_CHECK(cfg != nullptr, "LearnedChain: no step configuration");
    TORCH_CHECK(packed.is_cuda() && packed.is_contiguous() && packed.numel() >= cfg->P_total);
    if ((cfg->N & 3) || (cfg->F & 3)) donate = false;   // (the in-place kernel moves 16-byte pieces)
    if (at::GradMode::is_enabled() && packed.requires_grad()) {
      node = std::shared_ptr<LearnedChainNode>(new LearnedChainNode(), torch::autograd::deleteNode);
      node->packed = packed.detach();
      node->cfg = cfg;
      node->compact = donate;
      node->set_next_edges(torch::autograd::collect_next_edges(packed));
    }
  }
  bool executed() const { return node && node->executed; }
  bool recording() const { return node != nullptr; }
  int64_t steps() const { return node ? (int64_t)node->recs.size() : 0; }
  // cached steps (gcm_learned_step_cached): while the chain is linear, started from empty graphs, runs on a
  // donated state and has made fewer than N steps (no graph can have overflowed)
  bool cache_ok = false;
  // ... and past N steps, while the chain stays linear on its untouched donated state: every graph is full, the
  // steady-state step (gcm_learned_step_steady: one launch, the record of the two-launch form)
  bool steady_ok = false;
  int64_t cached_steps = 0, all_steps = 0, steady_steps = 0;
  at::Tensor cH, cA, cX;
  at::Tensor cU;                      // [B,N,F] W0b x_j of every stored row (gcm_learned_step_cached: cache_u)
  at::Tensor abits;                   // [B,N,4] the adjacency as bits, kept by the steady-state steps
  at::Tensor prev_rec;                // the previous steady step's record (its h1 / agg1 feed the next one)
  RecordPool rec_pool;                // the cached donated steps' records (small): sixteen per allocation
  const void* last_nodes = nullptr;   // the node matrix the previous step returned: a linear chain continues it
  // the state the previous step returned and its version counters right after the launch (the kernels write through
  // raw pointers: only a caller's in-place edit moves them, and the caches no longer describe such a state)
  at::Tensor l_nodes, l_adj, l_count;
  uint32_t lv_nodes = 0, lv_adj = 0, lv_count = 0;
  bool state_untouched(const at::Tensor& n, const at::Tensor& a, const at::Tensor& c) const {
    return l_nodes.defined() && n.unsafeGetTensorImpl() == l_nodes.unsafeGetTensorImpl() &&
           a.unsafeGetTensorImpl() == l_adj.unsafeGetTensorImpl() &&
           c.unsafeGetTensorImpl() == l_count.unsafeGetTensorImpl() && n._version() == lv_nodes &&
           a._version() == lv_adj && c._version() == lv_count;
  }
  int64_t n_cached() const { return cached_steps; }
};

struct LearnedStepOut {
  at::Tensor mx, nodes, adj, cur, count;
  int64_t index;   // of this step in the chain (or -1)
};
LearnedStepOut learned_step2_impl(LearnedChain& chain, const at::Tensor& obs_, const at::Tensor& nodes_in_,
                                  const at::Tensor& adj_in_, const at::Tensor& count_in, const at::Tensor& noise_,
                                  int64_t noise_is_exp, const at::Tensor& flags, int64_t parent, bool fresh) {
  LearnedCfg* cfg = chain.cfg;
  TORCH_CHECK(obs_.is_cuda() && nodes_in_.is_cuda() && adj_in_.is_cuda() && count_in.is_cuda() && noise_.is_cuda() &&
                  flags.is_cuda(),
              "learned_step: every tensor must live on a HIP device (no CPU fallback)");
  TORCH_CHECK(count_in.is_contiguous() && obs_.scalar_type() == at::kFloat && count_in.scalar_type() == at::kLong);
  at::Tensor obs = obs_.contiguous(), nodes_in = nodes_in_.contiguous(), adj_in = adj_in_.contiguous(),
             noise = noise_.contiguous();
  const int64_t B = obs.size(0);
  const int N = cfg->N, F = cfg->F, H1 = cfg->H1, H2 = cfg->H2;
  TORCH_CHECK(nodes_in.size(0) == B && nodes_in.size(1) == N && nodes_in.size(2) == F && adj_in.size(0) == B &&
                  adj_in.size(1) == N && adj_in.size(2) == N && count_in.size(0) == B && obs.size(1) == F &&
                  noise.numel() == B * N,
              "learned_step: hidden state, observation and noise shapes disagree");
  const bool need_bwd = chain.node != nullptr && at::GradMode::is_enabled();
  const bool donate = chain.donate;
  uint32_t* fl = reinterpret_cast<uint32_t*>(flags.data_ptr());
  const gcm_stream_t st = reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(obs.get_device()).stream());
  const float* pk = chain.packed.data_ptr<float>();
  const float* w_rel1 = pk;
  const float* w_root1 = w_rel1 + (size_t)H1 * F;
  const float* b1 = w_root1 + (size_t)H1 * F;
  const float* w_rel2 = b1 + H1;
  const float* w_root2 = w_rel2 + (size_t)H2 * H1;
  const float* b2 = w_root2 + (size_t)H2 * H1;
  if (need_bwd) TORCH_CHECK(parent < (int64_t)chain.node->recs.size());
  at::Tensor buf, nodes_out, adj_out, mx, cur, count_out;
  // cached step?  (see LearnedChain)
  if (chain.all_steps == 0)
    chain.cache_ok = fresh && (N & 3) == 0 && (F & 3) == 0 && nodes_in_.is_contiguous() && adj_in_.is_contiguous();
  else if (chain.cache_ok)
    chain.cache_ok = chain.last_nodes == nodes_in_.data_ptr() && chain.cached_steps == chain.all_steps &&
                     chain.cached_steps < N && (!need_bwd || parent == (int64_t)chain.node->recs.size() - 1) &&
                     chain.state_untouched(nodes_in_, adj_in_, count_in);
  const bool cached = chain.cache_ok;
  if (chain.all_steps == 0) chain.steady_ok = cached && donate;
  else if (chain.steady_ok && !cached)
    chain.steady_ok = chain.cached_steps == N && chain.all_steps == chain.cached_steps + chain.steady_steps &&
                      chain.last_nodes == nodes_in_.data_ptr() &&
                      (!need_bwd || parent == (int64_t)chain.node->recs.size() - 1) &&
                      chain.state_untouched(nodes_in_, adj_in_, count_in);
  const bool steady = !cached && donate && chain.steady_ok;
  if (cached) {
    if (chain.all_steps == 0) {
      // (no zero fill: a cached step reads rows < cur of the caches only, and the backward takes rows of a block that
      //  lie behind the candidates as zeros - three 4 MB fills less per chain)
      chain.cH = at::empty({B, N, H1}, obs.options());
      chain.cA = at::empty({B, N, F}, obs.options());
      chain.cX = at::empty({B, N, F}, obs.options());
      chain.cU = at::empty({B, N, F}, obs.options());   // (rows < cur are written before they are read as candidates)
      if (chain.node) {
        chain.node->cH = chain.cH; chain.node->cA = chain.cA; chain.node->cX = chain.cX;
        // (the cached steps write U at the exact shapes only: gcm_learned_step_cached)
        if (N == 128 && F == 32 && H1 == 32 && H2 == 32) chain.node->cU = chain.cU;
      }
    }
    size_t lay[8];
    check(gcm_learned_step_layout((int)B, N, F, H1, H2, donate ? 2 : 3, lay), "gcm_learned_step_layout");
    // (the donated step's record is small - adjacency row, belief, agg2, cur | count, soft row: sixteen per allocation;
    //  the functional step's holds the new state)
    buf = donate ? chain.rec_pool.take((int64_t)lay[0], obs, (int)obs.get_device()) : at::empty({(int64_t)lay[0]}, obs.options());
    float* base = buf.data_ptr<float>();
    int64_t* ib = reinterpret_cast<int64_t*>(base + lay[6]);
    if (!donate) {
      check(gcm_learned_step_cached_functional(
                obs.data_ptr<float>(), nodes_in.data_ptr<float>(), adj_in.data_ptr<float>(),
                count_in.data_ptr<int64_t>(), noise.data_ptr<float>(), (int)noise_is_exp, pk, cfg->has_bias, cfg->act1,
                cfg->act2, (float)cfg->eps0, (float)cfg->eps1, (float)cfg->cutoff, base, base + lay[1], ib, ib + B,
                base + lay[7], base + lay[2], base + lay[5], chain.cH.data_ptr<float>(), chain.cA.data_ptr<float>(),
                chain.cX.data_ptr<float>(), chain.cU.data_ptr<float>(), fl, (int)B, N, F, H1, H2,
                (int)chain.cached_steps, st),
            "gcm_learned_step_cached_functional");
      nodes_out = alias_of(buf, 0, {B, N, F}, buf.dtype());
      adj_out = alias_of(buf, (int64_t)lay[1], {B, N, N}, buf.dtype());
      count_out = alias_of(buf, (int64_t)lay[6] / 2 + B, {B}, caffe2::TypeMeta::Make<int64_t>());
    } else {
    // (GCM_LEARNED_FOUR_WAVES=1: the four-wave kernel where the eight-wave form exists - the A/B of tools and tests; a
    //  per-call flag of the C ABI, read from the environment by this host module once)
    static const int four_waves = (std::getenv("GCM_LEARNED_FOUR_WAVES") && std::getenv("GCM_LEARNED_FOUR_WAVES")[0] == '1')
                                      ? GCM_STEP_FOUR_WAVES : 0;
    check(gcm_learned_step_cached(obs.data_ptr<float>(), nodes_in.data_ptr<float>(), adj_in.data_ptr<float>(),
                                  count_in.data_ptr<int64_t>(), noise.data_ptr<float>(), (int)noise_is_exp, pk,
                                  cfg->has_bias | four_waves, cfg->act1, cfg->act2, (float)cfg->eps0, (float)cfg->eps1,
                                  (float)cfg->cutoff, ib, count_in.data_ptr<int64_t>(), base + lay[7], base + lay[1],
                                  base + lay[2], base + lay[5], chain.cH.data_ptr<float>(),
                                  chain.cA.data_ptr<float>(), chain.cX.data_ptr<float>(), chain.cU.data_ptr<float>(), fl,
                                  (int)B, N, F, H1, H2, (int)chain.cached_steps, st),
          "gcm_learned_step_cached");
    nodes_out = nodes_in_;
    adj_out = adj_in_;
    count_out = count_in;
    }
    mx = alias_of(buf, (int64_t)lay[2], {B, H2}, buf.dtype());
    cur = alias_of(buf, (int64_t)lay[6] / 2, {B}, caffe2::TypeMeta::Make<int64_t>());
    ++chain.cached_steps;
  } else if (donate) {
    // the state is advanced in place; the step's buffer keeps the node matrix after the insert, row cur of
    // the adjacency, the GNN's layers and the softmax row (gcm_learned_step_layout, compact)
    TORCH_CHECK(nodes_in_.is_contiguous() && adj_in_.is_contiguous(),
                "donate_state=True needs contiguous hidden-state tensors");
    size_t lay[8];
    check(gcm_learned_step_layout((int)B, N, F, H1, H2, 1, lay), "gcm_learned_step_layout");
    buf = at::empty({(int64_t)lay[0]}, obs.options());
    float* base = buf.data_ptr<float>();
    int64_t* ib = reinterpret_cast<int64_t*>(base + lay[6]);
    float* nodes = nodes_in.data_ptr<float>();
    float* adj = adj_in.data_ptr<float>();
    if (steady) {   // every graph is full: selection, in-place roll and the GNN of every row as ONE launch
      if (chain.steady_steps == 0) {   // the adjacency's bit image, carried along by the steady steps from here on
        chain.abits = at::empty({B, N, 4}, obs.options().dtype(at::kInt));
        check(gcm_adj_bits(adj, reinterpret_cast<uint32_t*>(chain.abits.data_ptr<int32_t>()), (int)B, N, st),
              "gcm_adj_bits");
      }
      // layer 1 of the rows as the previous step left it: its record, or the caches of the N cached steps
      const float* h1_prev = chain.steady_steps ? chain.prev_rec.data_ptr<float>() + lay[3] : chain.cH.data_ptr<float>();
      const float* agg1_prev = chain.steady_steps ? chain.prev_rec.data_ptr<float>() + lay[4] : chain.cA.data_ptr<float>();
      check(gcm_learned_step_steady(obs.data_ptr<float>(), nodes, adj, count_in.data_ptr<int64_t>(),
                                    noise.data_ptr<float>(), (int)noise_is_exp, pk, cfg->has_bias, cfg->act1, cfg->act2,
                                    (float)cfg->eps0, (float)cfg->eps1, (float)cfg->cutoff, ib,
                                    count_in.data_ptr<int64_t>(), base + lay[7], base, base + lay[1], base + lay[2],
                                    base + lay[3], base + lay[4], base + lay[5], h1_prev, agg1_prev,
                                    reinterpret_cast<uint32_t*>(chain.abits.data_ptr<int32_t>()), fl, (int)B, N, F, H1, H2, st),
            "gcm_learned_step_steady");
      chain.prev_rec = buf;
      ++chain.steady_steps;
    } else {
    check(gcm_learned_advance_select_inplace(obs.data_ptr<float>(), nodes, adj, count_in.data_ptr<int64_t>(),
                                             noise.data_ptr<float>(), (int)noise_is_exp, pk + cfg->P,
                                             (float)cfg->eps0, (float)cfg->eps1, (float)cfg->cutoff, ib,
                                             count_in.data_ptr<int64_t>(), base + lay[7], base, base + lay[1], fl,
                                             (int)B, N, F, st),
          "gcm_learned_advance_select_inplace");
    check(gcm_dense_gnn2_row_fwd(nodes, adj, ib, w_rel1, (cfg->has_bias & 1) ? b1 : nullptr, w_root1, cfg->act1,
                                 w_rel2, (cfg->has_bias & 2) ? b2 : nullptr, w_root2, cfg->act2, base + lay[2],
                                 base + lay[3], base + lay[4], base + lay[5], fl, (int)B, N, F, H1, H2, st),
          "gcm_dense_gnn2_row_fwd");
    }
    nodes_out = nodes_in_;
    adj_out = adj_in_;
    count_out = count_in;
    mx = alias_of(buf, (int64_t)lay[2], {B, H2}, buf.dtype());
    cur = alias_of(buf, (int64_t)lay[6] / 2, {B}, caffe2::TypeMeta::Make<int64_t>());
  } else {
    const Layout L(B, N, F, H1, H2, need_bwd);
    const int64_t o_soft = L.total;
    if (need_bwd) {
      size_t lay[8];
      check(gcm_learned_step_layout((int)B, N, F, H1, H2, 0, lay), "gcm_learned_step_layout");
      TORCH_CHECK((int64_t)lay[1] == L.o_adj && (int64_t)lay[2] == L.o_mx && (int64_t)lay[3] == L.o_h1 &&
                      (int64_t)lay[4] == L.o_agg1 && (int64_t)lay[5] == L.o_agg2 && (int64_t)lay[6] == L.o_idx &&
                      (int64_t)lay[7] == o_soft,
                  "learned_step: buffer layouts of the host node and the library disagree");
    }
    buf = at::empty({L.total + pad64(B * (int64_t)N)}, obs.options());
    float* base = buf.data_ptr<float>();
    int64_t* ib = reinterpret_cast<int64_t*>(base + L.o_idx);
    if ((N & 3) == 0 && (F & 3) == 0) {
      check(gcm_learned_advance_select_fused(obs.data_ptr<float>(), nodes_in.data_ptr<float>(),
                                             adj_in.data_ptr<float>(), count_in.data_ptr<int64_t>(),
                                             noise.data_ptr<float>(), (int)noise_is_exp, pk + cfg->P,
                                             (float)cfg->eps0, (float)cfg->eps1, (float)cfg->cutoff, base,
                                             base + L.o_adj, ib, ib + B, base + o_soft, fl, (int)B, N, F, st),
            "gcm_learned_advance_select_fused");
    } else {
      check(gcm_state_advance_fwd(nodes_in.data_ptr<float>(), adj_in.data_ptr<float>(), nullptr,
                                  count_in.data_ptr<int64_t>(), obs.data_ptr<float>(), base, base + L.o_adj, nullptr,
                                  ib, ib + B, fl, (int)B, N, F, st),
            "gcm_state_advance_fwd");
      check(gcm_learned_select_fused(base, base + L.o_adj, ib, noise.data_ptr<float>(), (int)noise_is_exp,
                                     pk + cfg->P, (float)cfg->eps0, (float)cfg->eps1, (float)cfg->cutoff,
                                     base + o_soft, (int)B, N, F, st),
            "gcm_learned_select_fused");
    }
    check(gcm_dense_gnn2_row_fwd(base, base + L.o_adj, ib, w_rel1, (cfg->has_bias & 1) ? b1 : nullptr, w_root1,
                                 cfg->act1, w_rel2, (cfg->has_bias & 2) ? b2 : nullptr, w_root2, cfg->act2,
                                 base + L.o_mx, need_bwd ? base + L.o_h1 : nullptr,
                                 need_bwd ? base + L.o_agg1 : nullptr, need_bwd ? base + L.o_agg2 : nullptr, fl,
                                 (int)B, N, F, H1, H2, st),
          "gcm_dense_gnn2_row_fwd");
    nodes_out = alias_of(buf, 0, {B, N, F}, buf.dtype());
    adj_out = alias_of(buf, L.o_adj, {B, N, N}, buf.dtype());
    mx = alias_of(buf, L.o_mx, {B, H2}, buf.dtype());
    cur = alias_of(buf, L.o_idx / 2, {B}, caffe2::TypeMeta::Make<int64_t>());
    count_out = alias_of(buf, L.o_idx / 2 + B, {B}, caffe2::TypeMeta::Make<int64_t>());
  }
  ++chain.all_steps;
  chain.last_nodes = nodes_out.data_ptr();
  chain.l_nodes = nodes_out;
  chain.l_adj = adj_out;
  chain.l_count = count_out;
  chain.lv_nodes = nodes_out._version();
  chain.lv_adj = adj_out._version();
  chain.lv_count = count_out._version();
  int64_t index = -1;
  if (need_bwd) {
    const c10::VariableVersion& vc = mx.unsafeGetTensorImpl()->version_counter();
    chain.node->recs.push_back({buf, vc, vc.current_version(), (int)parent, B, cached});
    index = (int64_t)chain.node->recs.size() - 1;
    torch::autograd::create_gradient_edge(mx, chain.node);
  }
  return {mx, nodes_out, adj_out, cur, count_out, index};
}
// -> (mx, nodes_out, adj_out, cur, count_out, index of this step in the chain (or -1))
pybind11::tuple learned_step2(LearnedChain& chain, const at::Tensor& obs, const at::Tensor& nodes_in,
                              const at::Tensor& adj_in, const at::Tensor& count_in, const at::Tensor& noise,
                              int64_t noise_is_exp, const at::Tensor& flags, int64_t parent, bool fresh) {
  LearnedStepOut r = learned_step2_impl(chain, obs, nodes_in, adj_in, count_in, noise, noise_is_exp, flags, parent,
                                        fresh);
  return pybind11::make_tuple(r.mx, r.nodes, r.adj, r.cur, r.count, r.index);
}

// ---------------------------------------------------------------------------------------------
// The packed parameter vector (gcm.py:_packed_params) as ONE autograd node: torch.cat of the flattened parameters
// with a backward that hands every parameter its slice of the flat gradient as a view - instead of CatBackward and a
// view node per parameter (six of them for the GNN, sixteen with the edge network: a third of a rollout's backward
// on the host).
// ---------------------------------------------------------------------------------------------
struct PackNode : public torch::autograd::Node {
  std::vector<std::vector<int64_t>> shapes;
  std::vector<int64_t> offs, ns;
  variable_list apply(variable_list&& grads) override {
    variable_list out(shapes.size());
    if (!grads[0].defined()) return out;
    const at::Tensor g = grads[0].contiguous();
    for (size_t i = 0; i < shapes.size(); ++i)
      if (task_should_compute_output(i)) out[i] = g.narrow(0, offs[i], ns[i]).view(shapes[i]);
    return out;
  }
};

// `packed` (built without history) as the output of a PackNode over `ts`, when any of them takes a gradient
static void hang_pack_node(at::Tensor& packed, const std::vector<at::Tensor>& ts) {
  bool any = false;
  for (const auto& t : ts) any = any || t.requires_grad();
  if (at::GradMode::is_enabled() && any) {
    auto node = std::shared_ptr<PackNode>(new PackNode(), torch::autograd::deleteNode);
    int64_t off = 0;
    for (const auto& t : ts) {
      node->shapes.push_back(t.sizes().vec());
      node->offs.push_back(off);
      node->ns.push_back(t.numel());
      off += t.numel();
    }
    node->set_next_edges(torch::autograd::collect_next_edges(ts));
    torch::autograd::create_gradient_edge(packed, node);   // (adds the input metadata itself)
  }
}

at::Tensor pack_params(const std::vector<at::Tensor>& ts) {
  TORCH_CHECK(!ts.empty());
  at::Tensor packed;
  {
    at::NoGradGuard ng;
    std::vector<at::Tensor> flat;
    flat.reserve(ts.size());
    for (const auto& t : ts) flat.push_back(t.reshape({-1}));
    packed = at::cat(flat);
  }
  hang_pack_node(packed, ts);
  return packed;
}

// pack_params, the cached step's weight image and the zero state of forward(x, None) as ONE launch
// (gcm_dense_rows_head_fused): -> (packed, image | None, nodes | None, adj | None, num_nodes | None).  want_image: the
// first six tensors are the GNN's (F, H1, H2 <= 64).  B > 0: the state DenseGCM._fresh_state carves - one allocation,
// nodes [B,N,feats] | adj [B,N,N] | num_nodes [B] (int64) at 64-float paddings, independent tensors (own version
// counters, no view relation).  The caller has checked: contiguous fp32 tensors on the current HIP device.
// fast / absorb: the RowsFast of the configuration (or None) and DenseGCM.rows_absorb_head && rows_merge_captured - under
// a stream capture the chain's run object then remembers this launch's node, and the chain's merged step node absorbs
// it (gcm_hip_run_head.h).
pybind11::tuple pack_params_head(const std::vector<at::Tensor>& ts, int F, int H1, int H2, bool want_image, int64_t B,
                                 int64_t N, int64_t feats, pybind11::object fast, bool absorb) {
  TORCH_CHECK(!ts.empty() && ts.size() <= 16, "pack_params_head: 1 .. 16 tensors");
  const at::Tensor& t0 = ts[0];
  std::vector<const float*> srcs;
  std::vector<size_t> lens;
  int64_t total = 0;
  for (const auto& t : ts) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.get_device() == t0.get_device(),
                "pack_params_head: contiguous float32 tensors on one HIP device");
    srcs.push_back(t.numel() ? t.data_ptr<float>() : nullptr);
    lens.push_back((size_t)t.numel());
    total += t.numel();
  }
  TORCH_CHECK(t0.get_device() == c10::hip::current_device(), "pack_params_head: tensors must live on the current device");
  const auto opts = t0.options().requires_grad(false);
  at::Tensor packed = at::empty({total}, opts), image, state, nodes, adj, count;
  if (want_image) image = at::empty({(int64_t)gcm_dense_rows_cached_weight_image_floats()}, opts);
  int64_t state_floats = 0;
  if (B > 0) {
    const int64_t n_nodes = pad64(B * N * feats), n_adj = pad64(B * N * N);
    state_floats = n_nodes + n_adj + 2 * B;
    state = at::empty({state_floats}, opts);
    nodes = alias_of(state, 0, {B, N, feats}, state.dtype());
    adj = alias_of(state, n_nodes, {B, N, N}, state.dtype());
    count = alias_of(state, (n_nodes + n_adj) / 2, {B}, caffe2::TypeMeta::Make<int64_t>());
  }
  void* run = fast.is_none() ? nullptr : fast.cast<RowsFast*>()->head_run(absorb && want_image && B > 0);
  check(gcm_dense_rows_head_fused_run(run, srcs.data(), lens.data(), (int)ts.size(), packed.data_ptr<float>(),
                                      want_image ? image.data_ptr<float>() : nullptr, F, H1, H2,
                                      B > 0 ? state.data_ptr() : nullptr, sizeof(float) * (size_t)state_floats,
                                      reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(t0.get_device()).stream())),
        "gcm_dense_rows_head_fused_run");
  hang_pack_node(packed, ts);
  auto opt = [](const at::Tensor& t) { return t.defined() ? pybind11::cast(t) : pybind11::object(pybind11::none()); };
  return pybind11::make_tuple(packed, opt(image), opt(nodes), opt(adj), opt(count));
}

// ---------------------------------------------------------------------------------------------
// The host path of a CONTINUING LearnedEdge chain (round 4; RowsFast's twin for gcm.py:_forward_learned): DenseGCM.__call__
// hands (obs, hidden) to step() directly, which validates what _forward_learned / _packed_params check in the
// interpreter every step - the hidden state is the one this chain returned last and no caller has written into it,
// same parameter objects at the same versions (read through the modules' own _parameters dicts), no hooks on the
// module, no injected noise function, grad mode unchanged, chain not yet run backward - draws the step's gumbel
// noise from the module's pool (the SAME list object _forward_learned uses: one RNG stream whichever path runs) and
// calls learned_step2.  Anything else returns None: the call then goes through nn.Module.__call__ and re-arms.
// ---------------------------------------------------------------------------------------------
struct LearnedFast {
  std::vector<pybind11::object> hook_dicts, dicts, keys, objs;
  std::vector<uint32_t> vers;
  pybind11::object sel_dict, key_noise;     // the selector module's __dict__ and the string "noise_fn"
  pybind11::object chain_obj, pool, link, root, weights;   // LearnedChain, gcm._noise_pool (list), the state's link items
  pybind11::object token, cfg_ref, flags_obj, key_link, key_lin;   // cfg_ref: weakref.ref(config) - the config owns this object
  LearnedChain* chain = nullptr;
  at::Tensor flags;
  bool armed = false, grad_mode = false;
  int dev = -1;
  int64_t xB = -1, xF = -1, parent = -1, N = 0, n_steps = 0;

  LearnedFast(const std::vector<std::pair<pybind11::object, pybind11::object>>& specs,
              const std::vector<pybind11::object>& hooks, pybind11::object sel_dict_)
      : hook_dicts(hooks), sel_dict(std::move(sel_dict_)) {
    for (const auto& sp : specs) {
      dicts.push_back(sp.first);
      keys.push_back(sp.second);
    }
    key_noise = pybind11::str("noise_fn");
    key_link = pybind11::str("_gcm_link");
    key_lin = pybind11::str("_gcm_lin");
  }
  bool hooks_registered() const {
    for (const auto& d : hook_dicts)
      if (PyObject_Size(d.ptr()) != 0) return true;
    return false;
  }
  bool params_current() const {
    for (size_t i = 0; i < dicts.size(); ++i) {
      PyObject* o = PyDict_GetItem(dicts[i].ptr(), keys[i].ptr());   // borrowed
      if (o != objs[i].ptr()) return false;
      if (o && THPVariable_Check(o) && THPVariable_Unpack(o)._version() != vers[i]) return false;
    }
    return true;
  }
  // after a step of _forward_learned on `chain_obj_`: the next call may come straight here
  void arm(pybind11::object chain_obj_, pybind11::object pool_, pybind11::object token_, pybind11::object cfg_,
           pybind11::object flags_, pybind11::object root_, pybind11::object weights_, int64_t parent_, int64_t xB_,
           int64_t xF_, int64_t N_) {
    chain_obj = std::move(chain_obj_);
    chain = &chain_obj.cast<LearnedChain&>();
    pool = std::move(pool_);
    token = std::move(token_);
    cfg_ref = std::move(cfg_);
    flags_obj = std::move(flags_);
    flags = THPVariable_Unpack(flags_obj.ptr());
    root = std::move(root_);
    weights = std::move(weights_);
    parent = parent_;
    xB = xB_; xF = xF_; N = N_;
    grad_mode = at::GradMode::is_enabled();
    dev = chain->packed.get_device();
    objs.clear();
    vers.clear();
    for (size_t i = 0; i < dicts.size(); ++i) {
      PyObject* o = PyDict_GetItem(dicts[i].ptr(), keys[i].ptr());
      objs.push_back(o ? pybind11::reinterpret_borrow<pybind11::object>(o) : pybind11::object());
      vers.push_back(o && THPVariable_Check(o) ? THPVariable_Unpack(o)._version() : 0);
    }
    armed = true;
  }
  void forget() {
    armed = false;
    chain = nullptr;
    chain_obj = pybind11::object();
    root = pybind11::object();
  }
  pybind11::object step(pybind11::handle x, pybind11::handle hidden) {
    if (!armed || !PyTuple_Check(hidden.ptr()) || PyTuple_GET_SIZE(hidden.ptr()) != 4 || !THPVariable_Check(x.ptr()))
      return pybind11::none();
    PyObject* h = hidden.ptr();
    PyObject *pn = PyTuple_GET_ITEM(h, 0), *pa = PyTuple_GET_ITEM(h, 1), *pw = PyTuple_GET_ITEM(h, 2),
             *pc = PyTuple_GET_ITEM(h, 3);
    if (!THPVariable_Check(pn) || !THPVariable_Check(pa) || !THPVariable_Check(pc) || pw != weights.ptr())
      return pybind11::none();
    const at::Tensor &tn = THPVariable_Unpack(pn), &ta = THPVariable_Unpack(pa), &tc = THPVariable_Unpack(pc);
    if (!chain->state_untouched(tn, ta, tc)) return pybind11::none();
    const at::Tensor& xt = THPVariable_Unpack(x.ptr());
    const bool grad = at::GradMode::is_enabled();
    if (grad != grad_mode || chain->executed() || xt.dim() != 2 || xt.size(0) != xB || xt.size(1) != xF ||
        xt.scalar_type() != at::kFloat || !xt.is_cuda() || xt.get_device() != dev || c10::hip::current_device() != dev ||
        (grad && xt.requires_grad()) || !params_current() || hooks_registered())
      return pybind11::none();
    PyObject* nf = PyDict_GetItem(sel_dict.ptr(), key_noise.ptr());
    if (nf != Py_None) return pybind11::none();   // (absent or injected: the interpreter's path decides)
    // the gumbel draws: DenseGCM.noise_pool_steps steps' worth per RNG launch, from the module's pool [tensor, next, capturing]
    if (!PyList_Check(pool.ptr()) || PyList_GET_SIZE(pool.ptr()) != 3) return pybind11::none();
    PyObject* pt = PyList_GET_ITEM(pool.ptr(), 0);
    if (!PyLong_Check(PyList_GET_ITEM(pool.ptr(), 1))) return pybind11::none();
    const long next = PyLong_AsLong(PyList_GET_ITEM(pool.ptr(), 1));
    const bool cap_now = c10::hip::currentStreamCaptureStatusMayInitCtx() != c10::hip::CaptureStatus::None;
    if (!THPVariable_Check(pt) || next < 0 || (PyList_GET_ITEM(pool.ptr(), 2) == Py_True) != cap_now)
      return pybind11::none();                     // (drawn under another capture state: refilled there)
    const at::Tensor& pool_t = THPVariable_Unpack(pt);
    if (pool_t.dim() != 3 || next >= pool_t.size(0) || pool_t.size(1) != xB || pool_t.size(2) != N || pool_t.get_device() != dev)
      return pybind11::none();                     // (exhausted: refilled on the interpreter's path)
    PyObject* cfg_live = PyWeakref_GetObject(cfg_ref.ptr());   // borrowed (the config owns this object: alive)
    if (!cfg_live || cfg_live == Py_None) return pybind11::none();
    // ---- nothing below declines: the step runs here ----
    at::Tensor noise = pool_t.select(0, next);
    PyObject* nx = PyLong_FromLong(next + 1);
    PyList_SetItem(pool.ptr(), 1, nx);            // (steals nx)
    LearnedStepOut r = learned_step2_impl(*chain, xt, tn, ta, tc, noise, 1, flags, parent, false);
    ++n_steps;
    const int64_t idx = r.index;
    parent = idx;
    pybind11::object pmx = pybind11::reinterpret_steal<pybind11::object>(THPVariable_Wrap(r.mx));
    if (chain->donate) {   // the state was advanced in place: the caller's own tensors and tuple
      if (idx >= 0) {
        pybind11::tuple lin = pybind11::make_tuple(chain_obj, idx);
        if (PyObject_SetAttr(pa, key_lin.ptr(), lin.ptr()) != 0) throw pybind11::error_already_set();
      }
      return pybind11::make_tuple(pmx, pybind11::reinterpret_borrow<pybind11::object>(h));
    }
    pybind11::object a2 = pybind11::reinterpret_steal<pybind11::object>(THPVariable_Wrap(r.adj)),
                     n2 = pybind11::reinterpret_steal<pybind11::object>(THPVariable_Wrap(r.nodes)),
                     c2 = pybind11::reinterpret_steal<pybind11::object>(THPVariable_Wrap(r.count));
    if (idx >= 0) {
      pybind11::tuple lin = pybind11::make_tuple(chain_obj, idx);
      if (PyObject_SetAttr(a2.ptr(), key_lin.ptr(), lin.ptr()) != 0) throw pybind11::error_already_set();
    }
    // functional state: what _forward_learned leaves on the new node matrix (gcm.py: `_gcm_link`)
    pybind11::object xshape = pybind11::reinterpret_steal<pybind11::object>(
        PyObject_GetAttrString(x.ptr(), "shape"));
    if (!xshape) throw pybind11::error_already_set();
    pybind11::tuple lk = pybind11::make_tuple(token, a2, pybind11::reinterpret_borrow<pybind11::object>(cfg_live),
                                              flags_obj, pybind11::none(), root, xshape, weights, c2);
    if (PyObject_SetAttr(n2.ptr(), key_link.ptr(), lk.ptr()) != 0) throw pybind11::error_already_set();
    return pybind11::make_tuple(pmx, pybind11::make_tuple(n2, a2, weights, c2));
  }
};

// ---------------------------------------------------------------------------------------------
// DenseGCM.rollout from EMPTY graphs with forward temporal hops as the only selectors, observations without gradient:
// the time-parallel forward (csrc/rollout_tp.hip: two launches for all T steps) and ONE autograd node whose backward
// is gcm_dense_rows_bptt_cached over the T records and the caches [B, Tc, .] (N := Tc).
// ---------------------------------------------------------------------------------------------
struct RowsRolloutNode : public torch::autograd::Node {
  at::Tensor packed, records, cH, cA, cX;
  c10::VariableVersion vc;
  uint32_t version = 0;
  int64_t T = 0, B = 0, Tc = 0, stride = 0;
  int F = 0, H1 = 0, H2 = 0, has_bias = 0, act1 = 0, act2 = 0;
  bool released = false;
  // from empty graphs, no resets, T <= N <= 128 (every row below T written by step t = row t, every hop a row of the
  // same graph): gcm_dense_rows_bptt_cached_hops with the trivial table
  bool hop_rows = false;
  bool hops_fold = true;   // StepCfg::hops_fold
  std::vector<gcm_selector_desc> descs;
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    TORCH_CHECK(!released, "Trying to backward through a DenseGCM.rollout a second time (its records were freed); "
                           "pass retain_graph=True to the first call");
    if (!grads[0].defined()) return out;
    TORCH_CHECK(vc.current_version() == version,
                "one of the variables needed for gradient computation has been modified by an inplace operation: "
                "the belief states returned by DenseGCM.rollout");
    at::Tensor g = grads[0].scalar_type() == at::kFloat ? grads[0] : grads[0].to(at::kFloat);
    std::vector<const float*> sv(T), gm(T);
    for (int64_t t = 0; t < T; ++t) {
      sv[t] = records.data_ptr<float>() + t * stride;
      gm[t] = g.data_ptr<float>() + t * g.stride(0);
    }
    const gcm_stream_t stream =
        reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(packed.get_device()).stream());
    const int64_t P = (int64_t)gcm_dense_gnn2_param_count(F, H1, H2);
    const size_t ws_bytes = std::max(gcm_dense_rows_bptt_workspace_bytes((int)T, (int)B, F, H1, H2),
                                     hop_rows ? sizeof(float) * (size_t)P * (size_t)B : (size_t)0);
    at::Tensor ws = at::empty({(int64_t)ws_bytes}, packed.options().dtype(at::kByte));
    at::Tensor res = packed.numel() > P ? at::zeros({packed.numel()}, packed.options()) : at::empty({P}, packed.options());
    int hops_rc = GCM_EUNSUPPORTED;
    if (hop_rows) {
      std::vector<uint8_t> cur((size_t)T);
      for (int64_t t = 0; t < T; ++t) cur[t] = (uint8_t)t;
      hops_rc = (hops_fold ? gcm_dense_rows_bptt_cached_hops : gcm_dense_rows_bptt_cached_hops_unfolded)(
                                                sv.data(), gm.data(), (int)T, (long)g.stride(1), (long)g.stride(2),
                                                packed.data_ptr<float>(), has_bias, act1, act2, cX.data_ptr<float>(),
                                                cH.data_ptr<float>(), cA.data_ptr<float>(), cur.data(),
                                                descs.empty() ? nullptr : descs.data(), (int)descs.size(), (int)T, nullptr,
                                                res.data_ptr<float>(), ws.data_ptr(), ws_bytes, (int)B, (int)Tc, F, H1, H2,
                                                stream);
    }
    if (hops_rc != GCM_EUNSUPPORTED) check(hops_rc, "gcm_dense_rows_bptt_cached_hops");
    else
    check(gcm_dense_rows_bptt_cached(sv.data(), gm.data(), (int)T, (long)g.stride(1), (long)g.stride(2),
                                     packed.data_ptr<float>(), has_bias, act1, act2, cX.data_ptr<float>(),
                                     cH.data_ptr<float>(), cA.data_ptr<float>(), nullptr, res.data_ptr<float>(),
                                     ws.data_ptr(), ws_bytes, (int)B, (int)Tc, F, H1, H2, stream),
          "gcm_dense_rows_bptt_cached");
    out[0] = res;
    return out;
  }
  void release_variables() override {
    records.reset(); cH.reset(); cA.reset(); cX.reset();
    released = true;
  }
  std::string name() const override { return "GcmRowsRollout"; }
};

// -> (mx_all [T,B,H2], nodes [B,N,F], adj [B,N,N], count [B]) or None when the configuration has no such form.
// reset (bool [T,B] on the device, optional): graph b is emptied before step t where reset[t,b] - the forward of
// csrc/rollout_reset.hip (episode starts in one launch, then the two time-parallel launches with the validity of a hop
// decided per graph); same records, same node, same backward.
pybind11::object rows_rollout_tp(int64_t cfg_handle, const at::Tensor& packed, const at::Tensor& obs_,
                                 const at::Tensor& flags, const c10::optional<at::Tensor>& reset_) {
  StepCfg* cfg = reinterpret_cast<StepCfg*>(cfg_handle);
  TORCH_CHECK(cfg != nullptr && obs_.is_cuda() && packed.is_cuda() && flags.is_cuda(),
              "rows_rollout_tp: every tensor must live on a HIP device (no CPU fallback)");
  at::Tensor obs = obs_.contiguous();
  const int64_t T = obs.size(0), B = obs.size(1);
  const int N = cfg->N, F = cfg->F, H1 = cfg->H1, H2 = cfg->H2;
  TORCH_CHECK(obs.dim() == 3 && obs.size(2) == F && obs.scalar_type() == at::kFloat && packed.is_contiguous() && T >= 1);
  // EuclideanEdge alone (csrc/euclid_tp.hip): every step's decisions as one causal contraction per graph, then the GNN of
  // all T <= N steps in one launch per graph; same records, same node
  const bool euclid = cfg->descs.size() == 1 && cfg->descs[0].kind == GCM_SEL_DISTANCE &&
                      cfg->descs[0].mode == GCM_DIST_EUCLID_CROSSBATCH && !cfg->descs[0].bidirectional &&
                      cfg->descs[0].cur_rows == nullptr && !(cfg->has_bias & ~3) && T <= N && B <= 65535 &&
                      gcm_euclid_rollout_tp_supported((int)T, (int)B, N, F, H1, H2);
  const bool with_reset = reset_.has_value() && reset_->defined();
  if (with_reset) {
    TORCH_CHECK(reset_->is_cuda() && reset_->scalar_type() == at::kBool && reset_->dim() == 2 && reset_->size(0) == T &&
                    reset_->size(1) == B,
                "rows_rollout_tp: reset must be a bool tensor [T, B] on the device");
    if (euclid) return pybind11::none();   // (EuclideanEdge: the per-step loop)
  }
  if (T > 65535 || (!euclid && !gcm_dense_rollout_tp_supported(cfg->descs.empty() ? nullptr : cfg->descs.data(),
                                                               (int)cfg->descs.size(), cfg->has_bias, (int)T, N, F, H1, H2)))
    return pybind11::none();
  const bool need_bwd = at::GradMode::is_enabled() && packed.requires_grad();
  const int64_t Tc = T;
  size_t lay[5];
  check(gcm_dense_rows_cached_layout((int)B, (int)Tc, F, H1, H2, lay), "gcm_dense_rows_cached_layout");
  const int64_t stride = need_bwd ? (int64_t)lay[0] : pad64(B * H2);
  at::Tensor records = at::empty({T * stride}, obs.options());
  // (with resets a graph's final state may hold fewer than min(T, N) nodes: always zero-filled)
  at::Tensor nodes = ((T < N || with_reset) && !euclid) ? at::zeros({B, N, F}, obs.options()) : at::empty({B, N, F}, obs.options());
  at::Tensor adj = euclid ? at::empty({B, N, N}, obs.options()) : at::zeros({B, N, N}, obs.options());
  at::Tensor count = at::empty({B}, obs.options().dtype(at::kLong));
  at::Tensor cH = at::empty({B, Tc, H1}, obs.options()), cA = at::empty({B, Tc, F}, obs.options()),
             cX = at::empty({B, Tc, F}, obs.options());
  at::Tensor mx_all = at::empty({T, B, H2}, obs.options());
  const gcm_stream_t st = reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(obs.get_device()).stream());
  if (euclid) {
    at::Tensor bits = at::empty({T, B, 4}, obs.options().dtype(at::kInt));
    check(gcm_euclid_rollout_tp_fwd(obs.data_ptr<float>(), cfg->descs[0].max_distance, cfg->descs[0].dist_param,
                                    packed.data_ptr<float>(), cfg->act1, cfg->act2, nodes.data_ptr<float>(),
                                    adj.data_ptr<float>(), count.data_ptr<int64_t>(), cH.data_ptr<float>(),
                                    cA.data_ptr<float>(), cX.data_ptr<float>(), records.data_ptr<float>(), (size_t)stride,
                                    need_bwd ? 1 : 0, mx_all.data_ptr<float>(), reinterpret_cast<uint32_t*>(bits.data_ptr()),
                                    reinterpret_cast<uint32_t*>(flags.data_ptr()), (int)T, (int)B, N, (int)Tc, F, H1, H2, st),
          "gcm_euclid_rollout_tp_fwd");
  } else if (with_reset) {
    at::Tensor reset = reset_->contiguous();
    at::Tensor start = at::empty({T, B}, obs.options().dtype(at::kInt));
    check(gcm_episode_start(reinterpret_cast<const uint8_t*>(reset.data_ptr()), start.data_ptr<int32_t>(), (int)T, (int)B, st),
          "gcm_episode_start");
    check(gcm_dense_rollout_tp_reset_fwd(obs.data_ptr<float>(), start.data_ptr<int32_t>(),
                                         cfg->descs.empty() ? nullptr : cfg->descs.data(), (int)cfg->descs.size(),
                                         packed.data_ptr<float>(), cfg->has_bias, cfg->act1, cfg->act2,
                                         nodes.data_ptr<float>(), adj.data_ptr<float>(), count.data_ptr<int64_t>(),
                                         cH.data_ptr<float>(), cA.data_ptr<float>(), cX.data_ptr<float>(),
                                         records.data_ptr<float>(), (size_t)stride, need_bwd ? 1 : 0,
                                         mx_all.data_ptr<float>(), reinterpret_cast<uint32_t*>(flags.data_ptr()), (int)T,
                                         (int)B, N, (int)Tc, F, H1, H2, st),
          "gcm_dense_rollout_tp_reset_fwd");
  } else
  check(gcm_dense_rollout_tp_fwd(obs.data_ptr<float>(), cfg->descs.empty() ? nullptr : cfg->descs.data(),
                                 (int)cfg->descs.size(), packed.data_ptr<float>(), cfg->has_bias, cfg->act1, cfg->act2,
                                 nodes.data_ptr<float>(), adj.data_ptr<float>(), count.data_ptr<int64_t>(),
                                 cH.data_ptr<float>(), cA.data_ptr<float>(), cX.data_ptr<float>(),
                                 records.data_ptr<float>(), (size_t)stride, need_bwd ? 1 : 0, mx_all.data_ptr<float>(),
                                 reinterpret_cast<uint32_t*>(flags.data_ptr()), (int)T, (int)B, N, (int)Tc, F, H1, H2, st),
        "gcm_dense_rollout_tp_fwd");
  if (need_bwd) {
    auto node = std::shared_ptr<RowsRolloutNode>(new RowsRolloutNode(), torch::autograd::deleteNode);
    node->packed = packed.detach();
    node->records = records; node->cH = cH; node->cA = cA; node->cX = cX;
    node->T = T; node->B = B; node->Tc = Tc; node->stride = stride;
    node->F = F; node->H1 = H1; node->H2 = H2; node->has_bias = cfg->has_bias; node->act1 = cfg->act1; node->act2 = cfg->act2;
    node->vc = mx_all.unsafeGetTensorImpl()->version_counter();
    node->version = node->vc.current_version();
    node->hop_rows = cfg->hops_bptt && !euclid && !with_reset && T <= N && T <= 128;
    if (node->hop_rows) node->descs = cfg->descs;
    node->hops_fold = cfg->hops_fold;
    node->set_next_edges(torch::autograd::collect_next_edges(packed));
    torch::autograd::create_gradient_edge(mx_all, node);
  }
  return pybind11::make_tuple(mx_all, nodes, adj, count);
}

// ---------------------------------------------------------------------------------------------
// DenseGCM.rollout with LearnedEdge from EMPTY graphs, T <= N steps, observations without gradient: the whole
// forward in three launches (gcm_learned_rollout_fwd: every (graph, step) independent work - the selection depends on raw
// observations and the given gumbel draws only), ONE autograd node whose backward is the chain's time-parallel one
// (gcm_learned_bptt_cached over the T records and the caches).  The returned state (nodes, adj, count) is new.
// ---------------------------------------------------------------------------------------------
struct LearnedRolloutNode : public torch::autograd::Node {
  at::Tensor packed, records, cH, cA, cX;
  c10::VariableVersion vc;
  uint32_t version = 0;
  LearnedCfg* cfg = nullptr;
  int64_t T = 0, B = 0, stride = 0;
  bool released = false;
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    TORCH_CHECK(!released, "Trying to backward through a DenseGCM.rollout (LearnedEdge) a second time (its records "
                           "were freed); pass retain_graph=True to the first call");
    if (!grads[0].defined()) return out;
    TORCH_CHECK(vc.current_version() == version,
                "one of the variables needed for gradient computation has been modified by an inplace operation: "
                "the belief states returned by DenseGCM.rollout (LearnedEdge)");
    at::Tensor g = grads[0].scalar_type() == at::kFloat ? grads[0] : grads[0].to(at::kFloat);
    const int N = cfg->N, F = cfg->F, H1 = cfg->H1, H2 = cfg->H2;
    std::vector<const float*> sv(T), gm(T);
    for (int64_t t = 0; t < T; ++t) {
      sv[t] = records.data_ptr<float>() + t * stride;
      gm[t] = g.data_ptr<float>() + t * g.stride(0);
    }
    const gcm_stream_t stream =
        reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(packed.get_device()).stream());
    const size_t ws_bytes = gcm_learned_bptt_workspace_bytes((int)T, (int)B, N, F, H1, H2);
    at::Tensor ws = at::empty({(int64_t)ws_bytes}, packed.options().dtype(at::kByte));
    at::Tensor res = at::empty({cfg->P_total}, packed.options());
    check(gcm_learned_bptt_cached(sv.data(), gm.data(), (int)T, (int)T, 2, cX.data_ptr<float>(), cH.data_ptr<float>(),
                                  cA.data_ptr<float>(), nullptr, (long)g.stride(1), (long)g.stride(2),
                                  packed.data_ptr<float>(),
                                  cfg->act1, cfg->act2, (float)cfg->eps0, (float)cfg->eps1, 1, nullptr,
                                  res.data_ptr<float>(), ws.data_ptr(), ws_bytes, (int)B, N, F, H1, H2, stream),
          "gcm_learned_bptt_cached");
    out[0] = res;
    return out;
  }
  void release_variables() override {
    records.reset(); cH.reset(); cA.reset(); cX.reset();
    released = true;
  }
  std::string name() const override { return "GcmLearnedRollout"; }
};

// -> (mx_all [T,B,H2], nodes [B,N,F], adj [B,N,N], count [B])
pybind11::tuple learned_rollout(int64_t cfg_handle, const at::Tensor& packed, const at::Tensor& obs_,
                                const at::Tensor& noise_, int64_t noise_is_exp, const at::Tensor& flags) {
  LearnedCfg* cfg = reinterpret_cast<LearnedCfg*>(cfg_handle);
  TORCH_CHECK(cfg != nullptr && obs_.is_cuda() && noise_.is_cuda() && packed.is_cuda() && flags.is_cuda(),
              "learned_rollout: every tensor must live on a HIP device (no CPU fallback)");
  at::Tensor obs = obs_.contiguous(), noise = noise_.contiguous();
  const int64_t T = obs.size(0), B = obs.size(1);
  const int N = cfg->N, F = cfg->F, H1 = cfg->H1, H2 = cfg->H2;
  TORCH_CHECK(obs.dim() == 3 && obs.size(2) == F && noise.numel() == T * B * N && T >= 1 && T <= N &&
                  packed.is_contiguous() && packed.numel() >= cfg->P_total && obs.scalar_type() == at::kFloat,
              "learned_rollout: shapes disagree (T <= graph_size steps from empty graphs)");
  const bool need_bwd = at::GradMode::is_enabled() && packed.requires_grad();
  size_t lay[8];
  check(gcm_learned_step_layout((int)B, N, F, H1, H2, 2, lay), "gcm_learned_step_layout");
  const int64_t stride = (int64_t)lay[0];
  at::Tensor records = at::empty({T * stride}, obs.options());
  at::Tensor nodes = at::zeros({B, N, F}, obs.options()), adj = at::zeros({B, N, N}, obs.options());
  at::Tensor count = at::empty({B}, obs.options().dtype(at::kLong));
  at::Tensor cH = at::empty({B, N, H1}, obs.options()), cA = at::empty({B, N, F}, obs.options()),
             cX = at::empty({B, N, F}, obs.options());
  at::Tensor mx_all = at::empty({T, B, H2}, obs.options());
  const gcm_stream_t st = reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(obs.get_device()).stream());
  check(gcm_learned_rollout_fwd(obs.data_ptr<float>(), noise.data_ptr<float>(), (int)noise_is_exp,
                                packed.data_ptr<float>(), cfg->has_bias, cfg->act1, cfg->act2, (float)cfg->eps0,
                                (float)cfg->eps1, (float)cfg->cutoff, nodes.data_ptr<float>(), adj.data_ptr<float>(),
                                count.data_ptr<int64_t>(), records.data_ptr<float>(), (size_t)stride,
                                cH.data_ptr<float>(), cA.data_ptr<float>(), cX.data_ptr<float>(),
                                mx_all.data_ptr<float>(), reinterpret_cast<uint32_t*>(flags.data_ptr()), (int)T, (int)B,
                                N, F, H1, H2, st),
        "gcm_learned_rollout_fwd");
  if (need_bwd) {
    auto node = std::shared_ptr<LearnedRolloutNode>(new LearnedRolloutNode(), torch::autograd::deleteNode);
    node->packed = packed.detach();
    node->records = records; node->cH = cH; node->cA = cA; node->cX = cX;
    node->cfg = cfg; node->T = T; node->B = B; node->stride = stride;
    node->vc = mx_all.unsafeGetTensorImpl()->version_counter();
    node->version = node->vc.current_version();
    node->set_next_edges(torch::autograd::collect_next_edges(packed));
    torch::autograd::create_gradient_edge(mx_all, node);
  }
  return pybind11::make_tuple(mx_all, nodes, adj, count);
}

// ---------------------------------------------------------------------------------------------
// SparseGCM.forward (sparse_gcm.py:72-212) for the canonical configuration - edge_selectors = TemporalEdge,
// gnn = 2 x GraphConv (+ fused activation), no preprocessor / positional encoder / aux selectors / max_hops -
// as ONE host call and ONE autograd node: plan -> (the one readback: flat sizes) -> insert -> temporal edges
// -> segmented merge with the stored COO list -> flatten -> CSR -> two GraphConv layers -> extract.
// Round 2 ran this from Python: ~35 launches and ~30 small torch ops per call, 0.21 ms of kernels inside
// 0.6 ms of wall time at cfg4, and 1.3 M states/s stepwise.
// ---------------------------------------------------------------------------------------------
// The GNN parameter gradients of the SparseGCM calls of one backward pass are summed here (one multi-tensor add
// per call) and handed to the parameters once, by a gate that is older than every call's node and therefore
// runs after all of them - not as one gradient tensor per call and parameter for the engine to add up (six
// small add kernels per call: 10 % of the GPU time of a stepwise run).
struct SparseGate : public torch::autograd::Node {
  std::vector<at::Tensor> acc = std::vector<at::Tensor>(6);
  std::vector<c10::TensorImpl*> keys = std::vector<c10::TensorImpl*>(6, nullptr);
  at::Tensor kick;      // a defined gradient for the gate's only input, so that it is certain to run
  int pass = -2;
  bool executed = false, gave = false;

  void begin_pass_if_new() {
    const int id = torch::autograd::get_current_graph_task_id();
    if (id == pass) return;
    pass = id;
    for (auto& a : acc) a = at::Tensor();
    gave = false;
  }
  void add(std::vector<at::Tensor>& g) {   // g[i] undefined: no gradient for that parameter
    std::vector<at::Tensor> dst, src;
    for (int i = 0; i < 6; ++i) {
      if (!g[i].defined()) continue;
      if (!acc[i].defined()) acc[i] = g[i];
      else { dst.push_back(acc[i]); src.push_back(g[i]); }
    }
    if (!dst.empty()) at::_foreach_add_(dst, src);
  }
  variable_list apply(variable_list&& grads) override {
    executed = true;
    variable_list out(6);
    if (pass == torch::autograd::get_current_graph_task_id())
      for (int i = 0; i < 6; ++i) out[i] = acc[i];
    for (auto& a : acc) a = at::Tensor();
    pass = -2;
    return out;
  }
  std::string name() const override { return "GcmSparseGate"; }
};

static std::shared_ptr<SparseGate>& sparse_gate_slot() {
  static std::shared_ptr<SparseGate> g;
  return g;
}

struct SparseStepNode : public torch::autograd::Node {
  std::shared_ptr<SparseGate> gate;
  at::Tensor T, taus, node_off, flat, edge_index, row_ptr, out1, agg1, out2, agg2;
  at::Tensor col_ptr, csc_rows, csc_perm;   // the CSC view when the forward already made it (whole episodes from empty graphs)
  at::Tensor w_rel1, w_root1, w_rel2, w_root2;
  int64_t B = 0, N = 0, F = 0, H1 = 0, H2 = 0, t_pad = 0, M = 0, E = 0;
  int act1 = 0, act2 = 0;
  bool has_b1 = false, has_b2 = false;
  // whole-episode calls (see sparse_temporal_step): the returned rows are out2 itself / the flat matrix is the state
  bool all_new = false, flat_is_state = false;
  c10::VariableVersion mx_vc;      // version counter of the returned rows when they alias out2, and its value then
  uint32_t mx_version = 0;
  c10::VariableVersion flat_vc;    // ... of the returned node matrix when the flat matrix aliases it (flat_is_state)
  uint32_t flat_version = 0;

  // inputs: x, nodes_in, the gate; outputs: mx_dense, nodes_out
  variable_list apply(variable_list&& grads) override {
    variable_list out(3);
    std::vector<at::Tensor> pg(6);   // w_rel1, b1, w_root1, w_rel2, b2, w_root2
    TORCH_CHECK(flat.defined(), "Trying to backward through a SparseGCM step a second time (its saved tensors "
                                "were freed); pass retain_graph=True to the first call");
    if (!grads[0].defined() && !grads[1].defined()) return out;
    // (the flat matrix layer 1's weight gradient reads IS the node matrix handed back to the caller)
    TORCH_CHECK(!flat_is_state || flat_vc.current_version() == flat_version,
                "one of the variables needed for gradient computation has been modified by an inplace operation: the node "
                "matrix returned by this SparseGCM call (every graph full: it is the flat matrix its backward reads) - "
                "edit a clone, or edit it after backward()");
    const auto opt = flat.options();
    const gcm_stream_t st = reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(flat.get_device()).stream());
    const bool need_x = task_should_compute_output(0), need_nodes = task_should_compute_output(1);
    const bool need_in = need_x || need_nodes;
    at::Tensor g_dirty;   // gradient w.r.t. the node matrix after the insert
    if (grads[1].defined()) g_dirty = grads[1].to(at::kFloat).contiguous();
    if (grads[0].defined()) {
      at::Tensor g_mx = grads[0].to(at::kFloat).contiguous();
      at::Tensor g_f2;
      if (all_new) {   // mx is out2 seen as [B, t_pad, H2]: its gradient is g_f2 as it is
        TORCH_CHECK(mx_vc.current_version() == mx_version,
                    "one of the variables needed for gradient computation has been modified by an inplace operation: "
                    "the rows returned by this SparseGCM call are the last layer's output its backward reads");
        g_f2 = g_mx.view({M, H2});
      } else {
        g_f2 = at::empty({M, H2}, opt);
        check(gcm_sparse_extract_bwd(g_mx.data_ptr<float>(), T.data_ptr<int64_t>(), taus.data_ptr<int64_t>(),
                                     node_off.data_ptr<int64_t>(), g_f2.data_ptr<float>(), (int)B, (int)t_pad,
                                     (int)H2, M, st),
              "gcm_sparse_extract_bwd");
      }
      // CSC view for the transpose gathers (grouped by graph: no sort)
      at::Tensor col_ptr = this->col_ptr, rows = csc_rows, perm = csc_perm;
      const int64_t* col = edge_index.data_ptr<int64_t>();
      if (E > 0 && !col_ptr.defined()) {
        col_ptr = at::empty({M + 1}, edge_index.options());
        rows = at::empty({E}, edge_index.options());
        perm = at::empty({E}, edge_index.options());
        check(gcm_csc_from_csr_batched(row_ptr.data_ptr<int64_t>(), col, col + E, node_off.data_ptr<int64_t>(),
                                       col_ptr.data_ptr<int64_t>(), rows.data_ptr<int64_t>(),
                                       perm.data_ptr<int64_t>(), (int)B, M, E, (int)N, st),
              "gcm_csc_from_csr_batched");
      }
      auto layer_bwd = [&](const at::Tensor& g_out, const at::Tensor& o, const at::Tensor& xin, const at::Tensor& ag,
                           const at::Tensor& w_rel, const at::Tensor& w_root, int Fi, int Fo, int act, bool want_x,
                           int i_rel, bool has_b) -> at::Tensor {
        at::Tensor g_xin = want_x ? at::empty({M, Fi}, opt) : at::Tensor();
        at::Tensor g_wr = at::empty_like(w_rel), g_wt = at::empty_like(w_root);
        at::Tensor g_b = has_b ? at::empty({Fo}, opt) : at::Tensor();
        const size_t wsb = gcm_csr_graphconv_bwd_workspace_bytes(M, Fi, Fo);
        at::Tensor ws = at::empty({(int64_t)wsb}, opt.dtype(at::kByte));
        check(gcm_csr_graphconv_bwd(g_out.data_ptr<float>(), o.data_ptr<float>(), xin.data_ptr<float>(),
                                    ag.data_ptr<float>(), row_ptr.data_ptr<int64_t>(), col,
                                    E > 0 ? col_ptr.data_ptr<int64_t>() : nullptr,
                                    E > 0 ? rows.data_ptr<int64_t>() : nullptr,
                                    E > 0 ? perm.data_ptr<int64_t>() : nullptr, nullptr, nullptr,
                                    w_rel.data_ptr<float>(), w_root.data_ptr<float>(),
                                    want_x ? g_xin.data_ptr<float>() : nullptr, nullptr, g_wr.data_ptr<float>(),
                                    has_b ? g_b.data_ptr<float>() : nullptr, g_wt.data_ptr<float>(), ws.data_ptr(),
                                    wsb, M, E, Fi, Fo, act, st),
              "gcm_csr_graphconv_bwd");
        pg[i_rel] = g_wr;
        if (has_b) pg[i_rel + 1] = g_b;
        pg[i_rel + 2] = g_wt;
        return g_xin;
      };
      at::Tensor g_f1 = layer_bwd(g_f2, out2, out1, agg2, w_rel2, w_root2, (int)H1, (int)H2, act2, true, 3, has_b2);
      at::Tensor g_flat = layer_bwd(g_f1, out1, flat, agg1, w_rel1, w_root1, (int)F, (int)H1, act1, need_in, 0, has_b1);
      gate->begin_pass_if_new();
      gate->add(pg);
      if (!gate->gave) {
        out[2] = gate->kick;
        gate->gave = true;
      }
      if (need_in) {
        at::Tensor g_nodes;
        if (flat_is_state) {
          g_nodes = g_flat.view({B, N, F});
        } else {
          g_nodes = at::empty({B, N, F}, opt);
          check(gcm_sparse_flatten_bwd(g_flat.data_ptr<float>(), T.data_ptr<int64_t>(), taus.data_ptr<int64_t>(),
                                       node_off.data_ptr<int64_t>(), g_nodes.data_ptr<float>(), (int)B, (int)N, (int)F,
                                       M, st),
                "gcm_sparse_flatten_bwd");
        }
        g_dirty = g_dirty.defined() ? g_dirty + g_nodes : g_nodes;
      }
    }
    if (need_in && g_dirty.defined()) {
      at::Tensor g_nodes_in = at::empty({B, N, F}, opt), g_x = at::empty({B, t_pad, F}, opt);
      check(gcm_sparse_insert_bwd(g_dirty.data_ptr<float>(), T.data_ptr<int64_t>(), taus.data_ptr<int64_t>(),
                                  g_nodes_in.data_ptr<float>(), g_x.data_ptr<float>(), (int)B, (int)N, (int)F,
                                  (int)t_pad, st),
            "gcm_sparse_insert_bwd");
      if (need_x) out[0] = g_x;
      if (need_nodes) out[1] = g_nodes_in;
    }
    return out;
  }
  void release_variables() override {
    flat.reset(); out1.reset(); agg1.reset(); out2.reset(); agg2.reset(); edge_index.reset(); row_ptr.reset();
  }
  std::string name() const override { return "GcmSparseStep"; }
};

// ---------------------------------------------------------------------------------------------
// SparseGCM called one node at a time (x [B, 1, F], taus in {0, 1}: ray_sparse_gcm.py's rollout loop), canonical
// configuration, in a chain of hidden states that started from EMPTY graphs.  TemporalEdge only ever points from a
// new node at older ones, so the layer-1 row of a node is final once written: the chain keeps h1 / agg1 / x of every
// node in caches and a call evaluates the new node's rows alone (gcm_sparse_step_cached: one launch) instead of
// flattening the batch, building CSR / CSC views and running both GraphConv layers over every stored node.  The
// state the caller sees (node matrix, COO adjacency, T) is advanced as before.  Backward: every cached call leaves
// a record; ONE gate per chain collects the records a backward pass reaches and runs one time-parallel launch over
// them (gcm_dense_rows_bptt_cached), handing each of the six parameter tensors its gradient once.
// ---------------------------------------------------------------------------------------------
struct SparseChainGate : public torch::autograd::Node {
  at::Tensor packed, cH, cA, cX, kick;
  std::vector<at::Tensor> recs, gms;   // what the current backward pass has reached
  int pass = -2;
  bool gave = false, executed = false, has_b1 = false, has_b2 = false;
  int B = 0, N = 0, F = 0, H1 = 0, H2 = 0, act1 = 0, act2 = 0;

  void begin_pass_if_new() {
    const int id = torch::autograd::get_current_graph_task_id();
    if (id == pass) return;
    pass = id;
    recs.clear();
    gms.clear();
    gave = false;
  }
  // inputs: the kick; outputs: w_rel1, b1, w_root1, w_rel2, b2, w_root2
  variable_list apply(variable_list&& grads) override {
    executed = true;
    variable_list out(6);
    const bool mine = pass == torch::autograd::get_current_graph_task_id();
    std::vector<at::Tensor> rs, gs;
    rs.swap(recs);
    gs.swap(gms);
    pass = -2;
    if (!mine || rs.empty()) return out;
    const int n = (int)rs.size();
    // incoming gradients [B, 1, H2]: by their own strides when every step's agree (slices of one stacked tensor,
    // expanded scalars), else as contiguous copies
    bool same = true;
    for (int i = 0; i < n; ++i)
      same = same && gs[i].scalar_type() == at::kFloat && gs[i].dim() == 3 && gs[i].stride(0) == gs[0].stride(0) &&
             gs[i].stride(2) == gs[0].stride(2);
    if (!same)
      for (int i = 0; i < n; ++i) gs[i] = gs[i].to(at::kFloat).contiguous();
    const long sb = (long)gs[0].stride(0), sh = (long)gs[0].stride(2);
    std::vector<const float*> sv(n), gm(n);
    for (int i = 0; i < n; ++i) { sv[i] = rs[i].data_ptr<float>(); gm[i] = gs[i].data_ptr<float>(); }
    const gcm_stream_t st =
        reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(packed.get_device()).stream());
    const size_t wsb = gcm_dense_rows_bptt_workspace_bytes(n, B, F, H1, H2);
    at::Tensor ws = at::empty({(int64_t)wsb}, packed.options().dtype(at::kByte));
    at::Tensor res = at::empty({packed.numel()}, packed.options());
    check(gcm_dense_rows_bptt_cached(sv.data(), gm.data(), n, sb, sh, packed.data_ptr<float>(),
                                     (has_b1 ? 1 : 0) | (has_b2 ? 2 : 0), act1, act2, cX.data_ptr<float>(),
                                     cH.data_ptr<float>(), cA.data_ptr<float>(), nullptr, res.data_ptr<float>(),
                                     ws.data_ptr(), wsb, B, N, F, H1, H2, st),
          "gcm_dense_rows_bptt_cached");
    // packed: W_rel1 | W_root1 | b1 | W_rel2 | W_root2 | b2
    int64_t o = 0;
    out[0] = res.narrow(0, o, (int64_t)H1 * F).view({H1, F}); o += (int64_t)H1 * F;
    out[2] = res.narrow(0, o, (int64_t)H1 * F).view({H1, F}); o += (int64_t)H1 * F;
    if (has_b1) out[1] = res.narrow(0, o, H1);
    o += H1;
    out[3] = res.narrow(0, o, (int64_t)H2 * H1).view({H2, H1}); o += (int64_t)H2 * H1;
    out[5] = res.narrow(0, o, (int64_t)H2 * H1).view({H2, H1}); o += (int64_t)H2 * H1;
    if (has_b2) out[4] = res.narrow(0, o, H2);
    return out;
  }
  std::string name() const override { return "GcmSparseChainGate"; }
};

struct SparseCachedStepNode : public torch::autograd::Node {
  std::shared_ptr<SparseChainGate> gate;
  at::Tensor rec;
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    TORCH_CHECK(rec.defined(), "Trying to backward through a SparseGCM step a second time (its saved tensors "
                               "were freed); pass retain_graph=True to the first call");
    if (!grads[0].defined()) return out;
    gate->begin_pass_if_new();
    gate->recs.push_back(rec);
    gate->gms.push_back(grads[0]);   // (as it comes - usually a slice of the caller's stacked beliefs: read by strides)
    if (!gate->gave) {
      out[0] = gate->kick;
      gate->gave = true;
    }
    return out;
  }
  void release_variables() override { rec.reset(); }
  std::string name() const override { return "GcmSparseCachedStep"; }
};

struct SparseChain {
  std::shared_ptr<SparseChainGate> gate;
  at::Tensor packed, wimg, cH, cA, cX;
  at::Tensor bptr;                           // per-graph pointer [B+1] of the COO list the previous call returned
  at::Tensor last_nodes, last_idx, last_T;   // the state the previous call returned (kept alive: its addresses
                                             // cannot be handed out again while the chain is armed)
  c10::TensorImpl* pkeys[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  uint32_t pvers[6] = {0, 0, 0, 0, 0, 0};
  uint32_t vers_nodes = 0, vers_T = 0;
  bool live = false;
  int64_t steps = 0, B = 0;

  void drop() {
    live = false;
    gate.reset();
    packed = wimg = cH = cA = cX = bptr = last_nodes = last_idx = last_T = at::Tensor();
  }
  bool same_params(const at::Tensor* const* ps) const {
    for (int i = 0; i < 6; ++i) {
      if ((ps[i] ? ps[i]->unsafeGetTensorImpl() : nullptr) != pkeys[i]) return false;
      if (ps[i] && ps[i]->_version() != pvers[i]) return false;
    }
    return true;
  }
  bool continues(const at::Tensor& nodes, const at::Tensor& idx, const at::Tensor& T,
                 const at::Tensor* const* ps) const {
    return live && last_nodes.defined() && nodes.data_ptr() == last_nodes.data_ptr() &&
           nodes._version() == vers_nodes && T.data_ptr() == last_T.data_ptr() && T._version() == vers_T &&
           idx.size(1) == last_idx.size(1) && (idx.size(1) == 0 || idx.data_ptr() == last_idx.data_ptr()) &&
           nodes.size(0) == B && same_params(ps);
  }
};

// -> (mx_dense [B,t,H2], nodes_out, indices [3,E] (batch, sink, source), values [E], T + taus), or an int status:
// 1 = overflow (sparse_gcm.py:120-121)
// the flat sizes of the last whole-episode call from empty graphs, by the taus tensor they were computed from
struct SizesMemo {
  at::Tensor taus;          // (held: its TensorImpl cannot be recycled while it is the key)
  uint32_t version = 0;
  std::vector<int> hops;
  int64_t N = 0;
  int64_t v[5] = {0, 0, 0, 0, 0};
  bool verify = false;      // this call used v[]: compare with the device's figures at the closing flag read
  int64_t hits = 0;         // calls that reused the sizes (tests)
};
static SizesMemo& sizes_memo() {
  static SizesMemo m;
  return m;
}
static at::Tensor& sizes_pinned() {   // edge_off[B] | M | n_new | max_total | max_tau (+ spare), pinned host memory
  static at::Tensor p;
  if (!p.defined()) p = at::empty({8}, at::TensorOptions().dtype(at::kLong).pinned_memory(true));
  return p;
}

pybind11::object sparse_temporal_step(const at::Tensor& x_, const at::Tensor& taus,
                                      const c10::optional<at::Tensor>& nodes_opt, int64_t N_arg,
                                      const at::Tensor& adj_idx_, const at::Tensor& T, const std::vector<int>& hops_desc,
                                      const at::Tensor& w_rel1, const c10::optional<at::Tensor>& b1,
                                      const at::Tensor& w_root1, int act1, const at::Tensor& w_rel2,
                                      const c10::optional<at::Tensor>& b2, const at::Tensor& w_root2, int act2,
                                      const at::Tensor& flags, pybind11::object chain_obj, bool fresh,
                                      bool want_flags) {
  // nodes_opt empty: the call starts from hidden = None - empty graphs - and the all-zero node matrix [B, N_arg, F] is
  // neither materialised nor read (`fresh` is then true by construction)
  const bool no_nodes = !nodes_opt.has_value();
  TORCH_CHECK(x_.is_cuda() && taus.is_cuda() && (no_nodes || nodes_opt->is_cuda()) && T.is_cuda() && flags.is_cuda(),
              "sparse step: every tensor must live on a HIP device (no CPU fallback)");
  TORCH_CHECK(!no_nodes || (fresh && adj_idx_.size(1) == 0 && N_arg > 0), "sparse step: no node matrix, but not a fresh state");
  at::Tensor x = x_.contiguous(), nodes = no_nodes ? at::Tensor() : nodes_opt->contiguous(), adj_idx = adj_idx_.contiguous();
  const at::Tensor nodes_ = no_nodes ? at::Tensor() : *nodes_opt;
  const bool nodes_grad = !no_nodes && nodes_.requires_grad();
  const int64_t B = x.size(0), t_pad = x.size(1), F = x.size(2), N = no_nodes ? N_arg : nodes.size(1);
  const int64_t H1 = w_rel1.size(0), H2 = w_rel2.size(0), Ea = adj_idx.size(1);
  TORCH_CHECK((no_nodes || (nodes.size(0) == B && nodes.size(2) == F)) && taus.numel() == B && T.numel() == B &&
                  w_rel1.size(1) == F && w_rel2.size(1) == H1,
              "sparse step: shapes disagree");
  const float* nodes_ptr = no_nodes ? nullptr : nodes.data_ptr<float>();
  const auto iopt = T.options();
  const gcm_stream_t st = reinterpret_cast<gcm_stream_t>(c10::hip::getCurrentHIPStream(x.get_device()).stream());
  uint32_t* fl = reinterpret_cast<uint32_t*>(flags.data_ptr());
  const at::Tensor* ps[6] = {&w_rel1, b1.has_value() ? &*b1 : nullptr, &w_root1,
                             &w_rel2, b2.has_value() ? &*b2 : nullptr, &w_root2};
  const bool need_bwd = at::GradMode::is_enabled() &&
                        (x_.requires_grad() || nodes_grad || w_rel1.requires_grad() ||
                         w_root1.requires_grad() || w_rel2.requires_grad() || w_root2.requires_grad() ||
                         (b1.has_value() && b1->requires_grad()) || (b2.has_value() && b2->requires_grad()));
  // ---- a call on the chain's caches?  (see SparseChain: one node per graph, no gradient w.r.t. x / the node matrix,
  //      a chain from empty graphs - `fresh`: the caller vouches that T == 0 everywhere - whose previous call
  //      returned exactly this state, parameters untouched since its head)
  SparseChain* ch = chain_obj.is_none() ? nullptr : chain_obj.cast<SparseChain*>();
  bool cached = false;
  if (ch) {
    bool ok = t_pad == 1 && !x_.requires_grad() && !nodes_grad && (F == 32 || F == 64) &&
              (H1 == 32 || H1 == 64) && H2 > 0 && H2 <= 64 && hops_desc.size() <= 16 &&
              (size_t)B * N * 64 < ((size_t)1 << 31) && w_rel1.scalar_type() == at::kFloat;
    for (int h : hops_desc) ok = ok && h >= 1;
    if (ok && fresh && Ea == 0) {
      ch->drop();
      at::NoGradGuard ng;
      std::vector<at::Tensor> parts = {
          w_rel1.detach().reshape({-1}), w_root1.detach().reshape({-1}),
          b1.has_value() ? b1->detach().reshape({-1}) : at::zeros({H1}, x.options()),
          w_rel2.detach().reshape({-1}), w_root2.detach().reshape({-1}),
          b2.has_value() ? b2->detach().reshape({-1}) : at::zeros({H2}, x.options())};
      ch->packed = at::cat(parts);
      ch->wimg = at::empty({(int64_t)gcm_dense_rows_cached_weight_image_floats()}, x.options());
      check(gcm_dense_rows_cached_weight_image(ch->packed.data_ptr<float>(), ch->wimg.data_ptr<float>(), (int)F,
                                               (int)H1, (int)H2, st),
            "gcm_dense_rows_cached_weight_image");
      // (rows are read only behind a select on "written before": no zero fill)
      ch->cH = at::empty({B, N, H1}, x.options());
      ch->cA = at::empty({B, N, F}, x.options());
      ch->cX = at::empty({B, N, F}, x.options());
      for (int i = 0; i < 6; ++i) {
        ch->pkeys[i] = ps[i] ? ps[i]->unsafeGetTensorImpl() : nullptr;
        ch->pvers[i] = ps[i] ? ps[i]->_version() : 0;
      }
      ch->B = B;
      ch->steps = 0;
      ch->live = cached = true;
    } else if (ok && !no_nodes && ch->continues(nodes, adj_idx, T, ps)) {
      cached = true;
    }
    if (!cached && ch->live) ch->drop();
  }
  std::vector<int32_t> hops(hops_desc.begin(), hops_desc.end());
  // (sizes and the flag word come back through a pinned host buffer: no pageable staging copy)
  static at::Tensor pinned_fl;
  at::Tensor& pinned = sizes_pinned();
  if (!pinned_fl.defined()) pinned_fl = at::empty({1}, at::TensorOptions().dtype(at::kInt).pinned_memory(true));
  at::Tensor host = pinned.narrow(0, 0, 5);   // edge_off[B] | M | n_new | max_total | max_tau
  const int64_t* hv = host.data_ptr<int64_t>();
  at::Tensor plan = at::empty({3 * (B + 1) + 4}, iopt);
  int64_t* node_off = plan.data_ptr<int64_t>();

  if (cached) {
    // ---- a call of the chain: five launches enqueued back to back, ONE readback at the end (sizes + flag word).
    //      The COO list is written into a buffer sized by the bound B * |hops| on the new entries (its rows E
    //      apart, E read on the device) and narrowed to the exact size afterwards.
    const int64_t max_new = B * (int64_t)hops.size();
    at::Tensor T_out = at::empty_like(T), bptr_out = at::empty({B + 1}, iopt);
    const int64_t* old_bptr = ch->bptr.defined() ? ch->bptr.data_ptr<int64_t>() : nullptr;
    TORCH_CHECK(Ea == 0 || old_bptr, "sparse chain: the stored list has no pointer");
    check(gcm_sparse_step_plan(T.data_ptr<int64_t>(), taus.data_ptr<int64_t>(), hops.data(), (int)hops.size(),
                               old_bptr, node_off, T_out.data_ptr<int64_t>(), bptr_out.data_ptr<int64_t>(), (int)B, st),
          "gcm_sparse_step_plan");
    // (the new node's rows first: they need the plan's inputs only - so that the sizes AND the flag word are on their
    //  way back while the state's copy and the COO list are still being written)
    size_t lay[5];
    check(gcm_dense_rows_cached_layout((int)B, (int)N, (int)F, (int)H1, (int)H2, lay), "gcm_dense_rows_cached_layout");
    at::Tensor rec = at::empty({need_bwd ? (int64_t)lay[0] : pad64(B * H2)}, x.options());
    at::Tensor mx = at::empty({B, t_pad, H2}, x.options());
    check(gcm_sparse_step_cached(x.data_ptr<float>(), T.data_ptr<int64_t>(), taus.data_ptr<int64_t>(), hops.data(),
                                 (int)hops.size(), ch->packed.data_ptr<float>(), ch->wimg.data_ptr<float>(), act1, act2,
                                 ch->cH.data_ptr<float>(), ch->cA.data_ptr<float>(), ch->cX.data_ptr<float>(),
                                 mx.data_ptr<float>(), rec.data_ptr<float>(), need_bwd ? 1 : 0, fl, (int)B, (int)N,
                                 (int)F, (int)H1, (int)H2, st),
          "gcm_sparse_step_cached");
    host.copy_(plan.narrow(0, 3 * (B + 1) - 1, 5), /*non_blocking=*/true);
    if (want_flags) pinned_fl.copy_(flags, /*non_blocking=*/true);
    static hipEvent_t events[64] = {};   // one per device (an event belongs to the device it was created on)
    const int dev_i = (int)x.get_device();
    TORCH_CHECK(dev_i >= 0 && dev_i < 64, "sparse chain: device index out of range");
    hipEvent_t& sizes_ready = events[dev_i];
    if (!sizes_ready)
      TORCH_CHECK(hipEventCreateWithFlags(&sizes_ready, hipEventDisableTiming) == hipSuccess, "hipEventCreate failed");
    TORCH_CHECK(hipEventRecord(sizes_ready, (hipStream_t)st) == hipSuccess, "hipEventRecord failed");
    at::Tensor nodes_out = at::empty({B, N, F}, x.options());
    check(gcm_sparse_insert_fwd(nodes_ptr, x.data_ptr<float>(), T.data_ptr<int64_t>(),
                                taus.data_ptr<int64_t>(), nodes_out.data_ptr<float>(), fl, (int)B, (int)N, (int)F,
                                (int)t_pad, st),
          "gcm_sparse_insert_fwd");
    at::Tensor idx_buf = at::empty({3 * (Ea + max_new)}, iopt), val_buf = at::empty({Ea + max_new}, x.options());
    check(gcm_sparse_chain_edges(Ea ? adj_idx.data_ptr<int64_t>() : nullptr, old_bptr, node_off,
                                 T.data_ptr<int64_t>(), taus.data_ptr<int64_t>(), hops.data(), (int)hops.size(),
                                 idx_buf.data_ptr<int64_t>(), val_buf.data_ptr<float>(), Ea, max_new, (int)B, st),
          "gcm_sparse_chain_edges");
    // the sizes and the flag word: as soon as the first two launches have retired - the others run on while the
    // host builds the outputs, returns and prepares the next call
    TORCH_CHECK(hipEventSynchronize(sizes_ready) == hipSuccess, "hipEventSynchronize failed");
    const int64_t Eb = hv[0], max_total = hv[3], E = Ea + Eb;
    if (max_total > N || Eb > max_new) {   // sparse_gcm.py:120-121 (every kernel above is bounds-checked)
      c10::hip::getCurrentHIPStream(x.get_device()).synchronize();
      ch->drop();
      flags.zero_();
      return pybind11::int_(1);
    }
    at::Tensor idx = idx_buf.narrow(0, 0, 3 * E).view({3, E}), vals = val_buf.narrow(0, 0, E);
    if (need_bwd) {
      if (!ch->gate) {
        auto g = std::shared_ptr<SparseChainGate>(new SparseChainGate(), torch::autograd::deleteNode);
        g->packed = ch->packed; g->cH = ch->cH; g->cA = ch->cA; g->cX = ch->cX;
        g->B = (int)B; g->N = (int)N; g->F = (int)F; g->H1 = (int)H1; g->H2 = (int)H2;
        g->act1 = act1; g->act2 = act2; g->has_b1 = b1.has_value(); g->has_b2 = b2.has_value();
        for (int i = 0; i < 6; ++i)
          g->add_next_edge(ps[i] && ps[i]->requires_grad() ? torch::autograd::impl::gradient_edge(*ps[i])
                                                           : torch::autograd::Edge());
        g->kick = at::zeros({1}, x.options());
        g->add_input_metadata(g->kick);
        ch->gate = g;
      }
      auto node = std::shared_ptr<SparseCachedStepNode>(new SparseCachedStepNode(), torch::autograd::deleteNode);
      node->gate = ch->gate;
      node->rec = rec;
      node->add_next_edge(torch::autograd::Edge(ch->gate, 0));
      torch::autograd::create_gradient_edge(mx, node);
    }
    ch->bptr = bptr_out;
    ch->last_nodes = nodes_out; ch->last_idx = idx; ch->last_T = T_out;
    ch->vers_nodes = nodes_out._version(); ch->vers_T = T_out._version();
    ++ch->steps;
    const int64_t bits = want_flags ? (int64_t)(uint32_t)pinned_fl.data_ptr<int32_t>()[0] : -1;
    return pybind11::make_tuple(mx, nodes_out, idx, vals, T_out, bits);
  }

  // ---- plan: node offsets, edge offsets; the one readback
  int64_t* new_off = node_off + (B + 1);
  int64_t* edge_off = new_off + (B + 1);
  int64_t* totals = edge_off + (B + 1);   // follows edge_off[B]: the five numbers read back are contiguous
  at::Tensor T_out;
  bool desc = !hops.empty() && hops.size() <= 16;
  for (size_t i = 1; i < hops.size(); ++i) desc = desc && hops[i] < hops[i - 1];
  if (desc) {   // offsets, totals, edge offsets and T + taus in one launch
    T_out = at::empty_like(T);
    check(gcm_sparse_step_plan(T.data_ptr<int64_t>(), taus.data_ptr<int64_t>(), hops.data(), (int)hops.size(), nullptr,
                               node_off, T_out.data_ptr<int64_t>(), nullptr, (int)B, st),
          "gcm_sparse_step_plan");
  } else {
    check(gcm_sparse_plan(T.data_ptr<int64_t>(), taus.data_ptr<int64_t>(), node_off, new_off, totals, (int)B, st),
          "gcm_sparse_plan");
    check(gcm_sparse_temporal_count(T.data_ptr<int64_t>(), taus.data_ptr<int64_t>(), hops.data(), (int)hops.size(),
                                    edge_off, (int)B, st),
          "gcm_sparse_temporal_count");
  }
  host.copy_(plan.narrow(0, 3 * (B + 1) - 1, 5), /*non_blocking=*/true);
  // The flat sizes are a pure function of (taus, T, hops).  Whole-episode calls from empty graphs (T = 0: `fresh`) with
  // the SAME taus tensor as the call before - same object, same version counter: a training loop's - reuse the sizes
  // that call read back, so nothing waits for the plan kernel and the call's launches are enqueued in one go (the
  // readback left the GPU idle for a third of a cfg4 call).  The device's own figures still travel to the pinned
  // buffer and are compared at the call's closing flag read (read_flag_word): a taus tensor written behind its
  // version counter's back raises there.  Only with the flag read at the end of the call (finite_check = "sync").
  SizesMemo& memo = sizes_memo();
  const bool memo_hit = want_flags && fresh && Ea == 0 && memo.taus.defined() &&
                        memo.taus.unsafeGetTensorImpl() == taus.unsafeGetTensorImpl() &&
                        memo.version == taus._version() && memo.hops == hops_desc && memo.N == N;
  int64_t sizes[5];
  if (memo_hit) {
    for (int i = 0; i < 5; ++i) sizes[i] = memo.v[i];
    memo.verify = true;    // (checked against hv[] once the stream has been synchronised)
    ++memo.hits;
  } else {
    c10::hip::getCurrentHIPStream(x.get_device()).synchronize();
    for (int i = 0; i < 5; ++i) sizes[i] = hv[i];
    memo.verify = false;
    if (want_flags && fresh && Ea == 0) {
      memo.taus = taus; memo.version = taus._version(); memo.hops = hops_desc; memo.N = N;
      for (int i = 0; i < 5; ++i) memo.v[i] = hv[i];
    } else {
      memo.taus = at::Tensor();
    }
  }
  const int64_t Eb = sizes[0], M = sizes[1], max_total = sizes[3];
  if (max_total > N) return pybind11::int_(1);
  at::Tensor node_off_t = plan.narrow(0, 0, B + 1);
  // What the packing kernels reduce to on whole episodes (the one-shot use, cfg4):
  //   from_empty    every graph starts empty (the caller vouches: `fresh`, no stored entries): the incoming node
  //                 matrix is all zeros and is not read;
  //   all_new       ... and every graph receives t_pad nodes: flat row i IS new node i, so the returned rows are the
  //                 last layer's output as it is (no extract copy forward, none backward);
  //   flat_is_state every graph is full after the call: the flat node matrix [M, F] IS the returned node matrix
  //                 [B, N, F] (no flatten copy).
  const bool from_empty = fresh && Ea == 0;
  const bool all_new = from_empty && M == B * t_pad && gcm_csr_graphconv_fwd_checked_supported(M, (int)H1, (int)H2) != 0;
  const bool flat_is_state = M == B * N;
  // ---- insert, edges, merge
  at::Tensor nodes_out = at::empty({B, N, F}, x.options());
  check(gcm_sparse_insert_fwd(from_empty ? nullptr : nodes_ptr, x.data_ptr<float>(), T.data_ptr<int64_t>(),
                              taus.data_ptr<int64_t>(), nodes_out.data_ptr<float>(), fl, (int)B, (int)N, (int)F,
                              (int)t_pad, st),
        "gcm_sparse_insert_fwd");
  at::Tensor idx_new = at::empty({3, Eb}, iopt), vals_new = at::empty({Eb}, x.options());
  // from empty graphs every index structure of the call is closed form: COO entries, unit weights, the flat list,
  // CSR pointers and (for the backward) the CSC view in ONE launch
  at::Tensor edge_index, row_ptr, col_ptr, csc_rows, csc_perm;
  bool structured = false;
  if (from_empty && Eb > 0) {
    bool ok = hops.size() <= 16;
    for (size_t i = 0; i < hops.size(); ++i) ok = ok && hops[i] >= 1 && (i == 0 || hops[i] < hops[i - 1]);
    if (ok) {
      edge_index = at::empty({2, Eb}, iopt);
      row_ptr = at::empty({M + 1}, iopt);
      if (need_bwd) {
        col_ptr = at::empty({M + 1}, iopt);
        csc_rows = at::empty({Eb}, iopt);
        csc_perm = at::empty({Eb}, iopt);
      }
      check(gcm_sparse_temporal_structure(taus.data_ptr<int64_t>(), hops.data(), (int)hops.size(), node_off, edge_off,
                                          idx_new.data_ptr<int64_t>(), vals_new.data_ptr<float>(),
                                          edge_index.data_ptr<int64_t>(), row_ptr.data_ptr<int64_t>(),
                                          need_bwd ? col_ptr.data_ptr<int64_t>() : nullptr,
                                          need_bwd ? csc_rows.data_ptr<int64_t>() : nullptr,
                                          need_bwd ? csc_perm.data_ptr<int64_t>() : nullptr, Eb, M, (int)B, st),
            "gcm_sparse_temporal_structure");
      structured = true;
    }
  }
  if (!structured)
    check(gcm_sparse_temporal_fill_vals(T.data_ptr<int64_t>(), taus.data_ptr<int64_t>(), hops.data(), (int)hops.size(),
                                        edge_off, idx_new.data_ptr<int64_t>(), vals_new.data_ptr<float>(), Eb, (int)B, st),
          "gcm_sparse_temporal_fill");
  at::Tensor idx, vals;
  if (Ea == 0) {
    idx = idx_new;
    vals = vals_new;
  } else if (Eb == 0) {
    idx = adj_idx;
  } else {
    at::Tensor old_bptr = at::empty({B + 1}, iopt);
    check(gcm_ptr_from_sorted(adj_idx.data_ptr<int64_t>(), old_bptr.data_ptr<int64_t>(), Ea, B, st),
          "gcm_ptr_from_sorted");
    idx = at::empty({3, Ea + Eb}, iopt);
    vals = at::empty({Ea + Eb}, x.options());   // (unit weights: the merge writes them as it goes)
    check(gcm_coo_merge_segments(adj_idx.data_ptr<int64_t>(), idx_new.data_ptr<int64_t>(), nullptr, nullptr,
                                 old_bptr.data_ptr<int64_t>(), edge_off, idx.data_ptr<int64_t>(),
                                 vals.data_ptr<float>(), nullptr, fl, Ea, Eb, (int)B, st),
          "gcm_coo_merge_segments");
  }
  const int64_t E = idx.size(1);
  if (!vals.defined()) vals = at::ones({E}, x.options());
  // ---- flat node matrix, CSR, the two layers, the new rows
  at::Tensor flat;
  if (flat_is_state) {
    flat = nodes_out.view({M, F});
  } else {
    flat = at::empty({M, F}, x.options());
    check(gcm_sparse_flatten_fwd(nodes_out.data_ptr<float>(), T.data_ptr<int64_t>(), taus.data_ptr<int64_t>(), node_off,
                                 flat.data_ptr<float>(), (int)B, (int)N, (int)F, M, st),
          "gcm_sparse_flatten_fwd");
  }
  if (!structured) {
    edge_index = at::empty({2, E}, iopt);
    row_ptr = at::empty({M + 1}, iopt);
    check(gcm_sparse_edges_to_csr(idx.data_ptr<int64_t>(), node_off, edge_index.data_ptr<int64_t>(),
                                  row_ptr.data_ptr<int64_t>(), fl, E, M, (int)B, st),
          "gcm_sparse_edges_to_csr");
  }
  at::Tensor out1 = at::empty({M, H1}, x.options()), out2 = at::empty({M, H2}, x.options());
  at::Tensor agg1 = need_bwd ? at::empty({M, F}, x.options()) : at::Tensor();
  at::Tensor agg2 = need_bwd ? at::empty({M, H1}, x.options()) : at::Tensor();
  at::Tensor wr1 = w_rel1.contiguous(), wt1 = w_root1.contiguous(), wr2 = w_rel2.contiguous(), wt2 = w_root2.contiguous();
  const int64_t* col = edge_index.data_ptr<int64_t>();
  check(gcm_csr_graphconv_fwd(flat.data_ptr<float>(), row_ptr.data_ptr<int64_t>(), col, nullptr, nullptr,
                              wr1.data_ptr<float>(), b1.has_value() ? b1->data_ptr<float>() : nullptr,
                              wt1.data_ptr<float>(), out1.data_ptr<float>(), need_bwd ? agg1.data_ptr<float>() : nullptr,
                              M, (int)F, (int)H1, act1, st),
        "gcm_csr_graphconv_fwd");
  at::Tensor mx;
  if (all_new) {   // the returned rows ARE the layer's output: its epilogue makes the finite check (sparse_gcm.py:201-203)
    check(gcm_csr_graphconv_fwd_checked(out1.data_ptr<float>(), row_ptr.data_ptr<int64_t>(), col, nullptr, nullptr,
                                        wr2.data_ptr<float>(), b2.has_value() ? b2->data_ptr<float>() : nullptr,
                                        wt2.data_ptr<float>(), out2.data_ptr<float>(),
                                        need_bwd ? agg2.data_ptr<float>() : nullptr, M, (int)H1, (int)H2, act2, fl, st),
          "gcm_csr_graphconv_fwd_checked");
    mx = alias_of(out2, 0, {B, t_pad, H2}, out2.dtype());   // (no view relation: it gets this call's node below)
  } else {
    check(gcm_csr_graphconv_fwd(out1.data_ptr<float>(), row_ptr.data_ptr<int64_t>(), col, nullptr, nullptr,
                                wr2.data_ptr<float>(), b2.has_value() ? b2->data_ptr<float>() : nullptr,
                                wt2.data_ptr<float>(), out2.data_ptr<float>(), need_bwd ? agg2.data_ptr<float>() : nullptr,
                                M, (int)H1, (int)H2, act2, st),
          "gcm_csr_graphconv_fwd");
    mx = at::empty({B, t_pad, H2}, x.options());
    check(gcm_sparse_extract_fwd(out2.data_ptr<float>(), T.data_ptr<int64_t>(), taus.data_ptr<int64_t>(), node_off,
                                 mx.data_ptr<float>(), fl, (int)B, (int)t_pad, (int)H2, M, st),
          "gcm_sparse_extract_fwd");
  }
  if (need_bwd) {
    auto node = std::shared_ptr<SparseStepNode>(new SparseStepNode(), torch::autograd::deleteNode);
    node->T = T; node->taus = taus; node->node_off = node_off_t; node->flat = flat;
    node->edge_index = edge_index; node->row_ptr = row_ptr; node->out1 = out1; node->agg1 = agg1;
    node->out2 = out2; node->agg2 = agg2;
    node->w_rel1 = wr1.detach(); node->w_root1 = wt1.detach(); node->w_rel2 = wr2.detach(); node->w_root2 = wt2.detach();
    node->B = B; node->N = N; node->F = F; node->H1 = H1; node->H2 = H2; node->t_pad = t_pad; node->M = M; node->E = E;
    node->act1 = act1; node->act2 = act2; node->has_b1 = b1.has_value(); node->has_b2 = b2.has_value();
    node->all_new = all_new; node->flat_is_state = flat_is_state;
    node->col_ptr = col_ptr; node->csc_rows = csc_rows; node->csc_perm = csc_perm;   // (defined: made with the CSR view)
    // (the returned rows alias out2, which the backward reads: an in-place write by the caller must be noticed)
    node->mx_vc = mx.unsafeGetTensorImpl()->version_counter();
    node->mx_version = node->mx_vc.current_version();
    if (flat_is_state) {
      node->flat_vc = nodes_out.unsafeGetTensorImpl()->version_counter();
      node->flat_version = node->flat_vc.current_version();
    }
    auto edge = [](const at::Tensor& t) {
      return t.requires_grad() ? torch::autograd::impl::gradient_edge(t) : torch::autograd::Edge();
    };
    // the gate of these six parameter tensors (a new one once the previous has run)
    std::shared_ptr<SparseGate>& slot = sparse_gate_slot();
    bool same = slot && !slot->executed;
    for (int i = 0; same && i < 6; ++i) same = slot->keys[i] == (ps[i] ? ps[i]->unsafeGetTensorImpl() : nullptr);
    if (!same) {
      slot = std::shared_ptr<SparseGate>(new SparseGate(), torch::autograd::deleteNode);
      for (int i = 0; i < 6; ++i) {
        slot->keys[i] = ps[i] ? ps[i]->unsafeGetTensorImpl() : nullptr;
        slot->add_next_edge(ps[i] ? edge(*ps[i]) : torch::autograd::Edge());
      }
      slot->kick = at::zeros({1}, w_rel1.options());
      slot->add_input_metadata(slot->kick);
    }
    node->gate = slot;
    node->add_next_edge(edge(x_));
    node->add_next_edge(no_nodes ? torch::autograd::Edge() : edge(nodes_));
    node->add_next_edge(torch::autograd::Edge(slot, 0));
    torch::autograd::create_gradient_edge(mx, node);
    if (x_.requires_grad() || nodes_grad) torch::autograd::create_gradient_edge(nodes_out, node);
    else node->add_input_metadata(torch::autograd::Node::undefined_input{});
  }
  if (!T_out.defined()) T_out = T + taus;
  return pybind11::make_tuple(mx, nodes_out, idx, vals, T_out, (int64_t)-1);   // (-1: flag word not read)
}

// The device flag word through a pinned host buffer (Tensor.item() stages through pageable memory: about twice
// the latency, and this is on the path of every SparseGCM call with finite_check = "sync").
int64_t read_flag_word(const at::Tensor& flags) {
  TORCH_CHECK(flags.is_cuda() && flags.numel() == 1 && flags.scalar_type() == at::kInt);
  static at::Tensor pinned;
  if (!pinned.defined()) pinned = at::empty({1}, at::TensorOptions().dtype(at::kInt).pinned_memory(true));
  pinned.copy_(flags, /*non_blocking=*/true);
  c10::hip::getCurrentHIPStream(flags.get_device()).synchronize();
  SizesMemo& memo = sizes_memo();
  if (memo.verify) {   // the call reused the sizes of an earlier one (see sparse_temporal_step): the device's own figures
    memo.verify = false;
    const int64_t* hv = sizes_pinned().data_ptr<int64_t>();
    bool same = true;
    for (int i = 0; i < 5; ++i) same = same && hv[i] == memo.v[i];
    if (!same) {
      memo.taus = at::Tensor();
      TORCH_CHECK(false, "SparseGCM: `taus` was modified in place without moving its version counter (through .data?) "
                         "between two calls: the sizes of this call's tensors were taken from the call before");
    }
  }
  return (int64_t)(uint32_t)pinned.data_ptr<int32_t>()[0];
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "C++ autograd node of the fused DenseGCM step (host side of libgcm_hip.so)";
  pybind11::class_<StepCfg>(m, "StepCfg")
      .def(pybind11::init<int64_t, int, int, int, int, int, int, int, int>())
      .def("handle", [](StepCfg& c) { return reinterpret_cast<int64_t>(&c); })
      .def("update_descs", &StepCfg::update_descs)
      .def("set_cached_flags", [](StepCfg& c, int f) { c.cached_flags = f; })
      .def("set_hops_bptt", [](StepCfg& c, bool on) { c.hops_bptt = on; })
      .def("set_hops_fold", [](StepCfg& c, bool on) { c.hops_fold = on; })
      .def("set_col_cache", [](StepCfg& c, bool on) { c.col_cache = on; })
      .def("set_merge_captured", [](StepCfg& c, bool on, int cap) { c.merge_captured = on; c.merge_cap = cap; })
      .def("set_absorb_head", [](StepCfg& c, bool on) { c.absorb_head = on; })
      .def("set_run_mfma", [](StepCfg& c, bool on) { c.run_mfma = on; })
      .def("cached_launches", [](StepCfg& c, int B) {   // launches per cached step (0: no cached form)
        return gcm_dense_rows_cached_launches(c.descs.empty() ? nullptr : c.descs.data(), (int)c.descs.size(),
                                              c.has_bias | c.cached_flags, B, c.N, c.F, c.H1, c.H2);
      });
  m.def("fused_step", &fused_step);
  pybind11::class_<RowsFast>(m, "RowsFast")
      .def(pybind11::init<const std::vector<std::pair<pybind11::object, pybind11::object>>&,
                          const std::vector<pybind11::object>&>())
      .def("run", &RowsFast::run)
      .def("step", &RowsFast::step)
      .def("continues", &RowsFast::continues)
      .def("edited_dx_state", &RowsFast::edited_dx_state)
      .def("donates", [](RowsFast& f) { return f.donate; })
      .def("pending", &RowsFast::pending)
      .def("forget", &RowsFast::forget)
      .def("set_head_image", &RowsFast::set_head_image)
      .def("steps", [](RowsFast& f) { return f.n_steps; })
      .def("cached_steps", [](RowsFast& f) { return f.cached_steps - f.col_steps; })
      .def("rolled_steps", [](RowsFast& f) { return f.rolled_steps; })
      .def("col_steps", [](RowsFast& f) { return f.col_steps; })
      .def("merge_stats", &RowsFast::merge_stats)
      .def("head_absorbed", &RowsFast::head_absorbed)
      .def("run_mfma", &RowsFast::run_mfma)
      .def("has_chain", [](RowsFast& f) { return f.node != nullptr || f.dxc != nullptr; });
  pybind11::class_<LearnedCfg>(m, "LearnedCfg")
      .def(pybind11::init<int, int, int, int, int, int, int, double, double, double>())
      .def("handle", [](LearnedCfg& c) { return reinterpret_cast<int64_t>(&c); });
  pybind11::class_<LearnedChain>(m, "LearnedChain")
      .def(pybind11::init<int64_t, const at::Tensor&, bool>())
      .def("cached_steps", &LearnedChain::n_cached)
      .def("total_steps", [](LearnedChain& c) { return c.all_steps; })
      .def("steady_steps", [](LearnedChain& c) { return c.steady_steps; })
      .def("donates", [](LearnedChain& c) { return c.donate; })
      .def("executed", &LearnedChain::executed)
      .def("recording", &LearnedChain::recording)
      .def("steps", &LearnedChain::steps);
  m.def("learned_step2", &learned_step2);
  m.def("pack_params", &pack_params);
  m.def("pack_params_head", &pack_params_head, pybind11::arg("tensors"), pybind11::arg("F"), pybind11::arg("H1"),
        pybind11::arg("H2"), pybind11::arg("want_image"), pybind11::arg("B"), pybind11::arg("N"), pybind11::arg("feats"),
        pybind11::arg("fast") = pybind11::none(), pybind11::arg("absorb") = false);
  pybind11::class_<LearnedFast>(m, "LearnedFast")
      .def(pybind11::init<const std::vector<std::pair<pybind11::object, pybind11::object>>&,
                          const std::vector<pybind11::object>&, pybind11::object>())
      .def("arm", &LearnedFast::arm)
      .def("step", &LearnedFast::step)
      .def("forget", &LearnedFast::forget)
      .def("steps", [](LearnedFast& f) { return f.n_steps; });
  m.def("learned_rollout", &learned_rollout);
  m.def("rows_rollout_tp", &rows_rollout_tp, pybind11::arg("cfg_handle"), pybind11::arg("packed"), pybind11::arg("obs"),
        pybind11::arg("flags"), pybind11::arg("reset") = pybind11::none());
  pybind11::class_<SparseChain>(m, "SparseChain")
      .def(pybind11::init<>())
      .def("steps", [](SparseChain& c) { return c.steps; })
      .def("live", [](SparseChain& c) { return c.live; })
      .def("drop", &SparseChain::drop);
  m.def("sparse_temporal_step", &sparse_temporal_step);
  m.def("sparse_sizes_memo_hits", []() { return sizes_memo().hits; });
  m.def("read_flag_word", &read_flag_word);
#ifdef GCM_HOST_PROF
  m.def("host_prof", []() {
    std::vector<double> v(g_prof, g_prof + 8);
    v.push_back((double)g_prof_n);
    for (auto& x : g_prof) x = 0;
    g_prof_n = 0;
    return v;
  });
#endif
}
