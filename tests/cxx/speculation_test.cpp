// CPU check of the frame driver's visibility speculation (amrvolumerenderer_amd/csrc/
// avr_speculation.h): the state machine is fed the events the driver feeds it -- a frame begins,
// an observation arrives, a repair is noted, the frame is decided -- with 8 local boxes, the
// smallest count the driver considers.
//   speculation_test      runs all cases, prints "ok", exit code 0
#include <cstdio>
#include <string>
#include <vector>

#include "../../amrvolumerenderer_amd/csrc/avr_speculation.h"

namespace {

int failures = 0;
void expect(bool ok, const std::string& what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s\n", what.c_str());
    ++failures;
  }
}

using S = Speculation;
constexpr int kBoxes = 8;
const std::vector<int32_t> kOrderA = {3, 0, 5, 1, 7, 2, 6, 4};  // position -> box
const std::vector<int32_t> kOrderB = {2, 6, 0, 4, 3, 7, 1, 5};
const std::vector<int> kThree = {0, 1, 2};
const std::vector<int> kAll = {0, 1, 2, 3, 4, 5, 6, 7};

// what a march under `order` records when its rays sample `boxes`: flags by position
std::vector<uint8_t> flags_of(const std::vector<int32_t>& order, const std::vector<int>& boxes) {
  std::vector<uint8_t> flags(S::flag_bytes(kBoxes), 0);
  for (size_t position = 0; position < order.size(); ++position) {
    for (int box : boxes) {
      if (order[position] == box) flags[position] = 1;
    }
  }
  return flags;
}

std::vector<int32_t> positions_of(const std::vector<int32_t>& order, const std::vector<int>& boxes) {
  std::vector<int32_t> positions;
  for (size_t position = 0; position < order.size(); ++position) {
    for (int box : boxes) {
      if (order[position] == box) positions.push_back(static_cast<int32_t>(position));
    }
  }
  return positions;
}

bool flags_agree(const S& sp) {
  if (sp.flags.size() != S::flag_bytes(kBoxes)) return false;
  std::vector<uint8_t> want(sp.flags.size(), 0);
  for (int32_t position : sp.positions) want[static_cast<size_t>(position)] = 1;
  return want == sp.flags;
}

S machine(float worth_it = 0.85f, double min_saving_ms = 0.0) {
  S sp;
  sp.worth_it = worth_it;
  sp.min_saving_ms = min_saving_ms;
  return sp;
}

// One frame the way the driver plays it: the oldest observation in flight arrives (its march
// sampled `sampled`; null: none arrives), a repair is noted, the frame is decided, and its march
// is observed (`observe`) if the machine wants it and a slot is free.
S::Decision frame(S& sp, const std::vector<int32_t>& order, const std::vector<int>* sampled,
                  bool repair = false, bool observe = true, double cell_bytes = 2.0e9) {
  sp.begin_frame(kBoxes);
  const int arrived = sp.oldest_pending();
  if (sampled != nullptr && arrived >= 0) {
    sp.absorb(arrived, flags_of(sp.observations[arrived].order, *sampled).data());
  }
  if (repair) sp.note_repair();
  const int slot = sp.free_slot();
  const S::Decision decision = sp.decide(order.data(), kBoxes, cell_bytes, slot >= 0);
  if (observe && sp.observed(decision.mode, slot >= 0, &order)) sp.observe(slot, order);
  sp.previous_plan = &order;
  return decision;
}

// a machine made active on {0, 1, 2} in its second frame
S active_machine() {
  S sp = machine();
  frame(sp, kOrderA, nullptr);
  frame(sp, kOrderA, &kThree);
  return sp;
}

void activation() {
  S sp = machine();
  S::Decision d = frame(sp, kOrderA, nullptr);
  expect(d.mode == 1 && !d.restart_corun && sp.state == S::kDeciding, "activation: the first frame observes");
  expect(sp.observations[0].pending && sp.observations[0].frame == 1, "activation: observation in flight");
  d = frame(sp, kOrderA, &kThree);
  expect(sp.state == S::kActive && d.mode == 2 && d.restart_corun, "activation: kObserving -> kActive, mode 2, restart");
  expect(sp.positions == positions_of(kOrderA, kThree), "activation: positions of the three boxes in the order passed in");
  expect(sp.positions == std::vector<int32_t>({1, 3, 5}), "activation: positions 1, 3, 5");
  expect(flags_agree(sp), "activation: flags agree with positions");
  expect(sp.sampled_fraction == 3.0f / 8.0f, "activation: sampled fraction 3/8");
}

void rejection() {
  S sp = machine();
  frame(sp, kOrderA, nullptr);
  S::Decision d = frame(sp, kOrderA, &kAll);
  expect(sp.state == S::kRejected && d.mode == 0 && !d.restart_corun, "rejection: kRejected, mode 0, no restart");
  expect(sp.asleep_until == sp.frame + 512 && sp.sampled_fraction == 1.0f, "rejection: asleep 512 frames");
  const int64_t wake = sp.asleep_until;
  while (sp.frame + 1 < wake) {
    d = frame(sp, kOrderA, nullptr);
    if (sp.state != S::kRejected || d.mode != 0 || d.restart_corun) break;
  }
  expect(sp.frame == wake - 1 && sp.state == S::kRejected, "rejection: asleep until then");
  expect(sp.last_sampled[0] == 1, "rejection: what was sampled is kept while asleep");
  sp.begin_frame(kBoxes);
  d = sp.decide(kOrderA.data(), kBoxes, 2.0e9, /*slot_free=*/false);
  expect(sp.frame == wake && sp.state == S::kObserving && d.mode == 0 && !d.restart_corun, "rejection: wakes observing");
  expect(sp.last_sampled == std::vector<int64_t>(kBoxes, -1), "rejection: every last_sampled reset");
}

void saving_floor() {
  for (int large = 0; large < 2; ++large) {
    const double cell_bytes = large ? 2.0e9 : 2.0e8;  // 0.25 ms / 0.025 ms saved at 3 of 8 boxes
    S sp = machine(0.85f, 0.15);
    frame(sp, kOrderA, nullptr, false, true, cell_bytes);
    const S::Decision d = frame(sp, kOrderA, &kThree, false, true, cell_bytes);
    if (large) {
      expect(sp.state == S::kActive && d.mode == 2 && d.restart_corun, "saving floor: 0.25 ms is worth it");
    } else {
      expect(sp.state == S::kRejected && d.mode == 0 && !d.restart_corun, "saving floor: 0.025 ms is not");
    }
  }
}

void memory_and_emptied_set() {
  // box 0 is last sampled in frame 1; boxes 1 and 2 again in frame 10
  S sp = machine();
  const std::vector<int> later = {1, 2};
  frame(sp, kOrderA, nullptr);                       // frame 1, observed
  frame(sp, kOrderA, &kThree, false, false);         // frame 2: active
  while (sp.frame < 9) frame(sp, kOrderA, nullptr, false, false);
  sp.begin_frame(kBoxes);                            // frame 10, observed
  sp.decide(kOrderA.data(), kBoxes, 2.0e9, true);
  sp.observe(sp.free_slot(), kOrderA);
  frame(sp, kOrderA, &later, false, false);          // frame 11: it arrives
  expect(sp.last_sampled[0] == 1 && sp.last_sampled[1] == 10 && sp.last_sampled[2] == 10, "memory: by frame");
  S::Decision d{0, false};
  while (sp.frame < 1 + S::kSpecMemory) d = frame(sp, kOrderA, nullptr, false, false);
  expect(sp.frame == 25 && d.mode == 2 && sp.positions == positions_of(kOrderA, kThree), "memory: in the set through F + 24");
  d = frame(sp, kOrderA, nullptr, false, false);
  expect(sp.frame == 26 && d.mode == 2 && !d.restart_corun && sp.positions == positions_of(kOrderA, later) && flags_agree(sp),
         "memory: out of the set in F + 25");
  while (sp.frame < 10 + S::kSpecMemory) d = frame(sp, kOrderA, nullptr, false, false);
  expect(sp.state == S::kActive && d.mode == 2 && sp.positions.size() == 2, "emptied set: still two boxes in frame 34");
  d = frame(sp, kOrderA, nullptr, false, false);
  expect(sp.positions.empty() && sp.state == S::kRejected && d.mode == 0 && d.restart_corun,
         "emptied set: kRejected, restart");
  expect(sp.asleep_until == sp.frame + 512, "emptied set: asleep 512 frames");
}

void by_box_not_position() {
  S sp = machine();
  frame(sp, kOrderA, nullptr);  // observed under order A
  const S::Decision d = frame(sp, kOrderB, &kThree);
  expect(d.mode == 2 && sp.positions == positions_of(kOrderB, kThree) && flags_agree(sp), "by box: B's positions of the same boxes");
  expect(sp.positions == std::vector<int32_t>({0, 2, 6}), "by box: positions 0, 2, 6");
}

// plays an active machine's 32-frame window with `repairs` repairs in it; the last frame's decision
S::Decision window(S& sp, int repairs) {
  S::Decision d{0, false};
  for (int k = 0; k < 32; ++k) {
    expect(sp.state == S::kActive && sp.recent_frames == k, "back-off: inside the window");
    d = frame(sp, kOrderA, &kThree, /*repair=*/k < repairs);
    if (k < 31) expect(d.mode == 2 && !d.restart_corun, "back-off: nothing before the window ends");
  }
  return d;
}

// from asleep (kBackoff) to active again: sleeps, wakes observing, observes, activates
void sleep_and_reactivate(S& sp) {
  while (sp.state == S::kBackoff) frame(sp, kOrderA, &kThree);
  expect(sp.frame >= sp.asleep_until, "back-off: not woken early");
  for (int k = 0; k < 4 && sp.state != S::kActive; ++k) frame(sp, kOrderA, &kThree);
  expect(sp.state == S::kActive && sp.recent_frames == 0 && sp.recent_repairs == 0, "back-off: active again");
}

void backoff() {
  {
    S sp = active_machine();
    const S::Decision d = window(sp, 17);
    expect(sp.state == S::kBackoff && d.mode == 0 && d.restart_corun, "back-off: 17 of 32 suspend, restart");
    expect(sp.asleep_until == sp.frame + 64 && sp.next_backoff == 128, "back-off: asleep 64 frames");
    expect(sp.repaired_frames == 17, "back-off: repairs counted");
  }
  {
    S sp = active_machine();
    const S::Decision d = window(sp, 16);
    expect(sp.state == S::kActive && d.mode == 2 && !d.restart_corun, "back-off: 16 of 32 is not more than half");
    expect(sp.next_backoff == 64 && sp.recent_frames == 0 && sp.recent_repairs == 0, "back-off: the window starts over");
  }
  {
    S sp = active_machine();
    const int want[] = {64, 128, 256, 512, 1024, 2048, 4096, 4096, 4096};
    for (int sleep : want) {
      window(sp, 32);
      expect(sp.state == S::kBackoff && sp.asleep_until == sp.frame + sleep,
             "back-off: successive sleeps double to 4096 (" + std::to_string(sleep) + ")");
      sleep_and_reactivate(sp);
    }
  }
  {
    S sp = active_machine();
    window(sp, 32);
    sleep_and_reactivate(sp);
    expect(sp.next_backoff == 128, "back-off: the next one would be 128");
    window(sp, 1);
    expect(sp.state == S::kActive && sp.next_backoff == 128, "back-off: a window with a repair keeps it");
    window(sp, 0);
    expect(sp.state == S::kActive && sp.next_backoff == 64, "back-off: a window without repairs resets it to 64");
  }
}

void deciding() {
  S sp = machine();
  sp.begin_frame(kBoxes);
  S::Decision d = sp.decide(kOrderA.data(), kBoxes, 2.0e9, /*slot_free=*/false);
  expect(d.mode == 0 && sp.state == S::kObserving, "deciding: no mode 1 without a free slot");
  sp.begin_frame(kBoxes);
  d = sp.decide(kOrderA.data(), kBoxes, 2.0e9, /*slot_free=*/true);
  expect(d.mode == 1 && !d.restart_corun && sp.state == S::kDeciding, "deciding: mode 1, then kDeciding");
  sp.observe(sp.free_slot(), kOrderA);
  for (int k = 0; k < 3; ++k) {
    d = frame(sp, kOrderA, nullptr);
    expect(d.mode == 0 && sp.state == S::kDeciding, "deciding: mode 0 until the observation arrives");
  }
  expect(sp.oldest_pending() == 0 && sp.free_slot() == 1, "deciding: one observation in flight");
  sp.begin_frame(kBoxes);
  sp.absorb(0, flags_of(kOrderA, kThree).data());
  expect(sp.state == S::kObserving && sp.free_slot() == 0 && sp.oldest_pending() == -1, "deciding: arrived -> kObserving");
  // every slot taken: none free, the oldest is the first taken
  S full = machine();
  for (int k = 0; k < S::kObservations; ++k) {
    full.begin_frame(kBoxes);
    full.observe(S::kObservations - 1 - k, kOrderA);
  }
  expect(full.free_slot() == -1 && full.oldest_pending() == S::kObservations - 1, "deciding: slots run out, oldest first");
}

void forget() {
  S sp = machine();
  frame(sp, kOrderA, nullptr);
  sp.forget();
  expect(sp.observations[0].pending && sp.observations[0].stale && sp.state == S::kObserving, "forget: pending -> stale");
  sp.begin_frame(kBoxes);
  sp.absorb(0, flags_of(kOrderA, kAll).data());
  expect(sp.last_sampled == std::vector<int64_t>(kBoxes, -1) && sp.sampled_fraction == -1.0f,
         "forget: a stale observation changes nothing");
  expect(!sp.observations[0].pending && !sp.observations[0].stale, "forget: the slot is free again");

  S active = active_machine();
  active.observe(active.free_slot(), kOrderA);
  active.begin_frame(kBoxes + 1);
  expect(active.state == S::kObserving && active.last_sampled == std::vector<int64_t>(kBoxes + 1, -1),
         "forget: a changed box count restarts at kObserving");
  // an observation of the old count arrives: skipped by its size
  const int arrived = active.oldest_pending();
  expect(arrived >= 0, "forget: one in flight");
  active.absorb(arrived, flags_of(kOrderA, kAll).data());
  expect(active.last_sampled == std::vector<int64_t>(kBoxes + 1, -1), "forget: an observation of another size is skipped");
}

void observed_frames() {
  S sp = active_machine();
  const int plan_a = 0, plan_b = 0;
  sp.previous_plan = &plan_a;
  sp.last_repair = -1000;
  sp.frame = 41;
  expect(!sp.observed(2, true, &plan_a), "observed: a standing plan, frame 41, no repair: not observed");
  expect(sp.observed(2, true, &plan_b), "observed: another plan");
  expect(!sp.observed(2, false, &plan_b), "observed: never without a slot");
  expect(!sp.observed(0, true, &plan_b), "observed: never in mode 0");
  expect(sp.observed(1, true, &plan_a), "observed: mode 1 always");
  sp.frame = 40;
  expect(sp.observed(2, true, &plan_a), "observed: frame % 8 == 0");
  sp.frame = 41;
  sp.last_repair = 26;
  expect(sp.observed(2, true, &plan_a), "observed: 15 frames after a repair");
  sp.last_repair = 25;
  expect(!sp.observed(2, true, &plan_a), "observed: not 16 frames after it");
}

}  // namespace

int main() {
  activation();
  rejection();
  saving_floor();
  memory_and_emptied_set();
  by_box_not_position();
  backoff();
  deciding();
  forget();
  observed_frames();
  if (failures == 0) std::puts("ok");
  return failures == 0 ? 0 : 1;
}
