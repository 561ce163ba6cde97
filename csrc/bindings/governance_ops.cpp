// torch.ops.svoc.governance: batched update_proposition / vote_for_a_proposition (governance_track: with the
// per-oracle track record); find_address: batched lookup.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "svoc/address_lookup.hpp"
#include "svoc/governance.hpp"
#include "svoc/ops.hpp"

extern "C" int svoc_governance(const svoc::GovState* g, const svoc::GovAction* a, hipStream_t s);
extern "C" int svoc_find_address(const svoc::AddrLookup* p, hipStream_t s);

namespace svoc {
namespace {

void prep(const at::Tensor& admins, at::Tensor& oracle_addr, at::Tensor& votes, at::Tensor& prop_tag,
          at::Tensor& prop_idx, at::Tensor& prop_addr, const at::Tensor& inst, const at::Tensor& caller,
          const at::Tensor& kind, const at::Tensor& arg0, const at::Tensor& arg1, const at::Tensor& addr,
          at::Tensor& status, at::Tensor& applied, bool enable, int64_t majority, GovState& g, GovAction& a,
          const at::Tensor* order = nullptr) {
  // every tensor on admins' device, checked before any pointer is taken: the dispatcher picks the HIP
  // implementation when ANY argument is a device tensor, and a kernel must never read through a host pointer
  const auto dev = admins.device();
  auto chk = [&](const at::Tensor& t, at::ScalarType dt, const char* n) {
    TORCH_CHECK(t.device() == dev, "governance: ", n, " must be on ", dev, " (got ", t.device(), ")");
    TORCH_CHECK(t.scalar_type() == dt && t.is_contiguous(), n, ": wrong dtype or not contiguous");
  };
  chk(admins, at::kLong, "admins"); chk(oracle_addr, at::kLong, "oracle_addr");
  chk(votes, at::kLong, "votes"); chk(prop_tag, at::kChar, "prop_tag"); chk(prop_idx, at::kInt, "prop_idx");
  chk(prop_addr, at::kLong, "prop_addr"); chk(inst, at::kLong, "inst"); chk(caller, at::kLong, "caller");
  chk(kind, at::kInt, "kind"); chk(arg0, at::kInt, "arg0"); chk(arg1, at::kLong, "arg1"); chk(addr, at::kLong, "addr");
  chk(status, at::kInt, "status"); chk(applied, at::kByte, "applied");
  if (order) {
    chk(*order, at::kLong, "order");
    TORCH_CHECK(order->numel() == inst.numel(), "order: contiguous int64 [K]");
  }
  TORCH_CHECK(admins.dim() == 3 && admins.size(2) == 4, "admins: [B, A, 4]");
  TORCH_CHECK(oracle_addr.dim() == 3 && oracle_addr.size(2) == 4, "oracle_addr: [B, N, 4]");
  g.B = (int)admins.size(0); g.A = (int)admins.size(1); g.N = (int)oracle_addr.size(1);
  TORCH_CHECK(g.A <= 64, "at most 64 admins (bit-packed vote columns)");
  TORCH_CHECK(votes.numel() == (int64_t)g.B * g.A && prop_tag.numel() == votes.numel() &&
              prop_idx.numel() == votes.numel() && prop_addr.numel() == votes.numel() * 4, "proposition shapes");
  const int64_t K = inst.numel();
  TORCH_CHECK(caller.numel() == K * 4 && kind.numel() == K && arg0.numel() == K && arg1.numel() == K &&
              addr.numel() == K * 4 && status.numel() == K && applied.numel() == K, "action shapes");
  g.admins = admins.data_ptr<int64_t>();
  g.oracle_addr = oracle_addr.data_ptr<int64_t>();
  g.votes = (uint64_t*)votes.data_ptr<int64_t>();
  g.prop_tag = prop_tag.data_ptr<int8_t>();
  g.prop_idx = prop_idx.data_ptr<int32_t>();
  g.prop_addr = prop_addr.data_ptr<int64_t>();
  g.enable = enable ? 1 : 0;
  g.majority = (int)majority;
  a.inst = inst.data_ptr<int64_t>(); a.caller = caller.data_ptr<int64_t>(); a.kind = kind.data_ptr<int32_t>();
  a.arg0 = arg0.data_ptr<int32_t>(); a.arg1 = arg1.data_ptr<int64_t>(); a.addr = addr.data_ptr<int64_t>();
  a.status = status.data_ptr<int32_t>(); a.applied = applied.data_ptr<uint8_t>(); a.K = (int)K;
  if (order) a.order = order->data_ptr<int64_t>();
}

void governance_cpu(const at::Tensor& admins, at::Tensor oracle_addr, at::Tensor votes, at::Tensor prop_tag,
                    at::Tensor prop_idx, at::Tensor prop_addr, const at::Tensor& inst, const at::Tensor& caller,
                    const at::Tensor& kind, const at::Tensor& arg0, const at::Tensor& arg1, const at::Tensor& addr,
                    bool enable, int64_t majority, at::Tensor status, at::Tensor applied) {
  GovState g{}; GovAction a{};
  prep(admins, oracle_addr, votes, prop_tag, prop_idx, prop_addr, inst, caller, kind, arg0, arg1, addr, status,
       applied, enable, majority, g, a);
  for (int k = 0; k < a.K; ++k) a.status[k] = gov_apply_one(g, a, k);  // in order
}

void governance_hip(const at::Tensor& admins, at::Tensor oracle_addr, at::Tensor votes, at::Tensor prop_tag,
                    at::Tensor prop_idx, at::Tensor prop_addr, const at::Tensor& inst, const at::Tensor& caller,
                    const at::Tensor& kind, const at::Tensor& arg0, const at::Tensor& arg1, const at::Tensor& addr,
                    bool enable, int64_t majority, at::Tensor status, at::Tensor applied) {
  TORCH_CHECK(admins.device().is_cuda(), "governance: admins must be on the device of the other tensors (got ",
              admins.device(), ")");
  GovState g{}; GovAction a{};
  prep(admins, oracle_addr, votes, prop_tag, prop_idx, prop_addr, inst, caller, kind, arg0, arg1, addr, status,
       applied, enable, majority, g, a);
  auto stream = c10::hip::getCurrentHIPStream(admins.device().index()).stream();
  const int rc = svoc_governance(&g, &a, stream);
  TORCH_CHECK(rc == 0, "svoc_governance failed: ", rc);
}

// Ordered batches: any number of actions per instance, applied in submission order per instance.  `order`:
// the action indices sorted stably by instance (Governance.submit_batch sorts on the device).
void governance_seq_cpu(const at::Tensor& admins, at::Tensor oracle_addr, at::Tensor votes, at::Tensor prop_tag,
                        at::Tensor prop_idx, at::Tensor prop_addr, const at::Tensor& inst, const at::Tensor& caller,
                        const at::Tensor& kind, const at::Tensor& arg0, const at::Tensor& arg1, const at::Tensor& addr,
                        bool enable, int64_t majority, const at::Tensor& order, at::Tensor status, at::Tensor applied) {
  GovState g{}; GovAction a{};
  prep(admins, oracle_addr, votes, prop_tag, prop_idx, prop_addr, inst, caller, kind, arg0, arg1, addr, status,
       applied, enable, majority, g, a, &order);
  // `order` is checked and then left unused: the CPU applies the whole list in order (instances are independent)
  for (int k = 0; k < a.K; ++k) a.status[k] = gov_apply_one(g, a, k);
}

void governance_seq_hip(const at::Tensor& admins, at::Tensor oracle_addr, at::Tensor votes, at::Tensor prop_tag,
                        at::Tensor prop_idx, at::Tensor prop_addr, const at::Tensor& inst, const at::Tensor& caller,
                        const at::Tensor& kind, const at::Tensor& arg0, const at::Tensor& arg1, const at::Tensor& addr,
                        bool enable, int64_t majority, const at::Tensor& order, at::Tensor status, at::Tensor applied) {
  TORCH_CHECK(admins.device().is_cuda(), "governance_seq: admins must be on the device of the other tensors (got ",
              admins.device(), ")");
  GovState g{}; GovAction a{};
  prep(admins, oracle_addr, votes, prop_tag, prop_idx, prop_addr, inst, caller, kind, arg0, arg1, addr, status,
       applied, enable, majority, g, a, &order);
  auto stream = c10::hip::getCurrentHIPStream(admins.device().index()).stream();
  const int rc = svoc_governance(&g, &a, stream);
  TORCH_CHECK(rc == 0, "svoc_governance failed: ", rc);
}

// governance_track: governance / governance_seq over an engine that keeps a per-oracle track record (track.hpp).
// An applied replacement clears the seat's record; min_streak > 0 is the failing-only replacement rule.
// `order` as in governance_seq (the device applies each instance's run in order), or None: one action per instance.
void prep_track(const at::Tensor& admins, const at::Tensor& rounds, at::Tensor& flagged, at::Tensor& streak,
                at::Tensor& score, at::Tensor& since, int64_t min_streak, GovState& g) {
  const auto dev = admins.device();
  auto chk = [&](const at::Tensor& t, at::ScalarType dt, int64_t n, const char* name) {
    TORCH_CHECK(t.scalar_type() == dt && t.is_contiguous() && t.numel() == n && t.device() == dev,
                "governance_track: ", name, ": wrong dtype, shape or device, or not contiguous");
  };
  const int64_t BN = (int64_t)g.B * g.N;
  chk(rounds, at::kInt, g.B, "rounds"); chk(flagged, at::kInt, BN, "flagged"); chk(streak, at::kInt, BN, "streak");
  chk(score, at::kLong, BN, "score"); chk(since, at::kInt, BN, "since");
  TORCH_CHECK(min_streak >= 0 && min_streak <= 0x7fffffff, "governance_track: min_streak out of range");
  g.track_rounds = rounds.data_ptr<int32_t>();
  g.track_flagged = flagged.data_ptr<int32_t>();
  g.track_streak = streak.data_ptr<int32_t>();
  g.track_score = score.data_ptr<int64_t>();
  g.track_since = since.data_ptr<int32_t>();
  g.min_streak = (int)min_streak;
}

void governance_track_cpu(const at::Tensor& admins, at::Tensor oracle_addr, at::Tensor votes, at::Tensor prop_tag,
                          at::Tensor prop_idx, at::Tensor prop_addr, const at::Tensor& inst, const at::Tensor& caller,
                          const at::Tensor& kind, const at::Tensor& arg0, const at::Tensor& arg1, const at::Tensor& addr,
                          bool enable, int64_t majority, const c10::optional<at::Tensor>& order, at::Tensor status,
                          at::Tensor applied, const at::Tensor& rounds, at::Tensor flagged, at::Tensor streak,
                          at::Tensor score, at::Tensor since, int64_t min_streak) {
  (void)order;   // the CPU applies the whole list in order (instances are independent)
  TORCH_CHECK(admins.device().is_cpu(), "governance_track: admins must be a host tensor here");
  GovState g{}; GovAction a{};
  prep(admins, oracle_addr, votes, prop_tag, prop_idx, prop_addr, inst, caller, kind, arg0, arg1, addr, status,
       applied, enable, majority, g, a);
  prep_track(admins, rounds, flagged, streak, score, since, min_streak, g);
  for (int k = 0; k < a.K; ++k) a.status[k] = gov_apply_one(g, a, k);  // in order
}

void governance_track_hip(const at::Tensor& admins, at::Tensor oracle_addr, at::Tensor votes, at::Tensor prop_tag,
                          at::Tensor prop_idx, at::Tensor prop_addr, const at::Tensor& inst, const at::Tensor& caller,
                          const at::Tensor& kind, const at::Tensor& arg0, const at::Tensor& arg1, const at::Tensor& addr,
                          bool enable, int64_t majority, const c10::optional<at::Tensor>& order, at::Tensor status,
                          at::Tensor applied, const at::Tensor& rounds, at::Tensor flagged, at::Tensor streak,
                          at::Tensor score, at::Tensor since, int64_t min_streak) {
  TORCH_CHECK(admins.device().is_cuda(), "governance_track: admins must be on the device of the other tensors");
  GovState g{}; GovAction a{};
  prep(admins, oracle_addr, votes, prop_tag, prop_idx, prop_addr, inst, caller, kind, arg0, arg1, addr, status,
       applied, enable, majority, g, a);
  prep_track(admins, rounds, flagged, streak, score, since, min_streak, g);
  if (order.has_value() && order->defined()) {
    TORCH_CHECK(order->scalar_type() == at::kLong && order->is_contiguous() && order->numel() == inst.numel() &&
                order->device() == admins.device(), "order: contiguous int64 [K]");
    a.order = order->data_ptr<int64_t>();
  }
  auto stream = c10::hip::getCurrentHIPStream(admins.device().index()).stream();
  const int rc = svoc_governance(&g, &a, stream);
  TORCH_CHECK(rc == 0, "svoc_governance failed: ", rc);
}

// find_address: batched find_oracle_index / admin lookup (address_lookup.hpp).  Writes `out` in place: no
// allocation and no host synchronisation, so a captured graph replays it.
AddrLookup prep_lookup(const at::Tensor& table, const at::Tensor& inst, const at::Tensor& addr, at::Tensor& out) {
  auto chk = [&](const at::Tensor& t, const char* n) {
    TORCH_CHECK(t.device() == table.device(), "find_address: ", n, " must be on ", table.device(), " (got ",
                t.device(), ")");
    TORCH_CHECK(t.scalar_type() == at::kLong && t.is_contiguous(), "find_address: ", n, ": contiguous int64");
  };
  chk(table, "table"); chk(inst, "inst"); chk(addr, "addr"); chk(out, "out");
  TORCH_CHECK(table.dim() == 3 && table.size(2) == 4, "find_address: table: [B, M, 4]");
  TORCH_CHECK(table.size(1) < (int64_t(1) << 30), "find_address: table too wide");
  const int64_t K = inst.numel();
  TORCH_CHECK(inst.dim() == 1 && addr.dim() == 2 && addr.size(0) == K && addr.size(1) == 4 && out.dim() == 1 &&
              out.numel() == K, "find_address: inst [K], addr [K, 4], out [K]");
  AddrLookup p{};
  p.B = table.size(0); p.M = (int)table.size(1); p.K = K;
  if (K == 0) return p;
  p.table = table.data_ptr<int64_t>(); p.inst = inst.data_ptr<int64_t>(); p.addr = addr.data_ptr<int64_t>();
  p.out = out.data_ptr<int64_t>();
  return p;
}

void find_address_cpu(const at::Tensor& table, const at::Tensor& inst, const at::Tensor& addr, at::Tensor out) {
  TORCH_CHECK(table.device().is_cpu(), "find_address: table must be a host tensor here");
  const AddrLookup p = prep_lookup(table, inst, addr, out);
  for (int64_t k = 0; k < p.K; ++k) p.out[k] = find_address_one(p, k);
}

void find_address_hip(const at::Tensor& table, const at::Tensor& inst, const at::Tensor& addr, at::Tensor out) {
  // (the dispatcher comes here when ANY argument is a device tensor: a host tensor among them is refused by
  // prep_lookup before a kernel could read through its pointer)
  TORCH_CHECK(table.device().is_cuda(), "find_address: table must be on the device of the other tensors (got ",
              table.device(), ")");
  const AddrLookup p = prep_lookup(table, inst, addr, out);
  if (p.K == 0) return;
  // the kernel reads addresses as 16-B vectors
  TORCH_CHECK((((uintptr_t)p.table | (uintptr_t)p.addr) & 15) == 0, "find_address: table / addr not 16-B aligned");
  auto stream = c10::hip::getCurrentHIPStream(table.device().index()).stream();
  const int rc = svoc_find_address(&p, stream);
  TORCH_CHECK(rc == 0, "svoc_find_address failed: ", rc);
}

}  // namespace

void register_governance_defs(torch::Library& m) {
  m.def(
      "governance(Tensor admins, Tensor(a!) oracle_addr, Tensor(b!) votes, Tensor(c!) prop_tag, "
      "Tensor(d!) prop_idx, Tensor(e!) prop_addr, Tensor inst, Tensor caller, Tensor kind, Tensor arg0, "
      "Tensor arg1, Tensor addr, bool enable, int majority, Tensor(f!) status, Tensor(g!) applied) -> ()");
  m.def(
      "governance_seq(Tensor admins, Tensor(a!) oracle_addr, Tensor(b!) votes, Tensor(c!) prop_tag, "
      "Tensor(d!) prop_idx, Tensor(e!) prop_addr, Tensor inst, Tensor caller, Tensor kind, Tensor arg0, "
      "Tensor arg1, Tensor addr, bool enable, int majority, Tensor order, Tensor(f!) status, "
      "Tensor(g!) applied) -> ()");
  m.def(
      "governance_track(Tensor admins, Tensor(a!) oracle_addr, Tensor(b!) votes, Tensor(c!) prop_tag, "
      "Tensor(d!) prop_idx, Tensor(e!) prop_addr, Tensor inst, Tensor caller, Tensor kind, Tensor arg0, "
      "Tensor arg1, Tensor addr, bool enable, int majority, Tensor? order, Tensor(f!) status, "
      "Tensor(g!) applied, Tensor rounds, Tensor(h!) flagged, Tensor(i!) streak, Tensor(j!) score, "
      "Tensor(k!) since, int min_streak) -> ()");
  m.def("find_address(Tensor table, Tensor inst, Tensor addr, Tensor(a!) out) -> ()");
}
void register_governance_cpu(torch::Library& m) {
  m.impl("governance", &governance_cpu);
  m.impl("governance_seq", &governance_seq_cpu);
  m.impl("governance_track", &governance_track_cpu);
  m.impl("find_address", &find_address_cpu);
}
void register_governance_hip(torch::Library& m) {
  m.impl("governance", &governance_hip);
  m.impl("governance_seq", &governance_seq_hip);
  m.impl("governance_track", &governance_track_hip);
  m.impl("find_address", &find_address_hip);
}

}  // namespace svoc
