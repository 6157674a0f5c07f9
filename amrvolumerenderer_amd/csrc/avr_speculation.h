// The decisions of the frame driver's visibility speculation (avr_renderer.cpp), free of any GPU
// call so that they can be exercised on the CPU (tests/cxx/speculation_test.cpp).  The driver owns
// the HIP side -- the pinned observation buffers and their events, the visited / missed device
// buffers, the miss flag -- and feeds this class events, the way it feeds CoRunTuner.
#ifndef AVR_SPECULATION_H
#define AVR_SPECULATION_H

#include <algorithm>
#include <cstdint>
#include <vector>

// With the reference's default boxTransparency = 0 the march's skip test keeps config-4's rays out
// of 118 of its 176 boxes, yet every frame reads their f64 cells.  The driver remembers, per BOX
// of the rank, the last frame whose march sampled it (observations: a march that records the boxes
// it samples, the flags copied to the host and read a few frames later -- by box, so they outlive
// the plan: a moving camera keeps what it learnt).  While at most worth_it of the boxes were
// sampled in the last kSpecMemory frames, a frame classifies only those (a launch of exactly
// their tiles), its march checks every box it is about to march against the same set, and two
// gated launches behind it repair the frame when the set was wrong (the cells changed, the camera
// turned) -- results never change.  Config-4 opaque: classify pass 0.55 -> 0.18 ms, pipelined
// frame 0.64 -> 0.43 ms.  A translucent frame (every box sampled) is observed once and then left
// alone but for one observing frame in kSpecProbeEvery.
struct Speculation {
  static constexpr int kSpecMemory = 24;       // frames a box stays in the set after it was last sampled
  static constexpr int kSpecProbeEvery = 512;  // kRejected: one observing frame in so many
  static constexpr int kSpecObserveEvery = 8;  // kActive without repairs: one observed frame in so many
  float worth_it = 0.85f;        // (avr_renderer_debug_set_speculation_threshold: tests)
  double min_saving_ms = 0.15;   // (... sets it to 0 with any threshold: small test scenes)

  enum State { kObserving, kDeciding, kActive, kRejected, kBackoff };
  State state = kObserving;
  std::vector<int64_t> last_sampled;     // per local box: the last frame that sampled it (-1 never)
  std::vector<int32_t> positions;        // this frame's set, as positions in its layer order
  std::vector<uint8_t> flags;            // ... and as flags by position (staged with the march)
  int64_t frame = 0;                     // frames this struct has seen
  int64_t asleep_until = 0;              // kRejected / kBackoff: the next observing frame
  int next_backoff = 64;                 // after the next run of repairs
  int recent_repairs = 0, recent_frames = 0;
  int64_t last_repair = -1000;           // the frame that learnt of the latest repair
  const void* previous_plan = nullptr;   // of the frame before (only compared: a standing camera)
  // observations in flight: that frame's layer order (the march's flags by POSITION and the event
  // that says they have arrived are the driver's, slot by slot)
  struct Observation {
    std::vector<int32_t> order;          // position -> local box of that frame's plan
    int64_t frame = 0;
    bool pending = false;
    bool stale = false;                  // taken under settings that are gone: ignored when it arrives
  };
  static constexpr int kObservations = 4;
  Observation observations[kObservations];
  long active_frames = 0, repaired_frames = 0;
  float sampled_fraction = -1.0f;        // of the rank's boxes, in the last kSpecMemory frames

  // bytes of the flags of n_boxes positions (what the march stages: whole 16-byte words)
  static size_t flag_bytes(int n_boxes) { return (static_cast<size_t>(std::max(n_boxes, 1)) + 15) / 16 * 16; }

  void forget() {                        // (another transfer function, other boxes)
    last_sampled.clear();
    state = kObserving;
    sampled_fraction = -1.0f;
    for (Observation& o : observations) o.stale = o.pending;  // (their flags are of the old settings)
  }

  // A considered frame begins (every one: also when chunks later suppress the decision).
  void begin_frame(int n_boxes) {
    ++frame;
    if (last_sampled.size() != static_cast<size_t>(n_boxes)) {
      last_sampled.assign(static_cast<size_t>(n_boxes), -1);
      state = kObserving;
    }
  }

  // The observation in flight that was taken first (-1: none).  They arrive in that order.
  int oldest_pending() const {
    int oldest = -1;
    for (int k = 0; k < kObservations; ++k) {
      if (observations[k].pending && (oldest < 0 || observations[k].frame < observations[oldest].frame)) oldest = k;
    }
    return oldest;
  }

  // A slot for this frame's observation (-1: the host is far ahead, this frame is not observed).
  int free_slot() const {
    for (int k = 0; k < kObservations; ++k) {
      if (!observations[k].pending) return k;
    }
    return -1;
  }

  // Observation `slot` has arrived: `sampled` are the flags by position of its frame's march.
  void absorb(int slot, const uint8_t* sampled) {
    Observation& o = observations[slot];
    o.pending = false;
    if (state == kDeciding) state = kObserving;
    if (o.stale || o.order.size() != last_sampled.size()) {
      o.stale = false;
      return;
    }
    for (size_t position = 0; position < o.order.size(); ++position) {
      if (sampled[position] != 0) {
        int64_t& last = last_sampled[static_cast<size_t>(o.order[position])];
        last = std::max(last, o.frame);
      }
    }
    sampled_fraction = -2.0f;  // (to be counted by decide())
  }

  // This frame's march records what it samples into observation `slot`, under layer order `order`.
  void observe(int slot, const std::vector<int32_t>& order) {
    Observation& o = observations[slot];
    o.order = order;
    o.frame = frame;
    o.pending = true;
  }

  // A march of an earlier frame missed (its repair redid that frame).
  void note_repair() {
    ++repaired_frames;
    ++recent_repairs;
    last_repair = frame;
  }

  // What this frame does: mode 0 nothing, 1 a plain frame whose march records the boxes it samples,
  // 2 classifies only the set, checks, repairs -- and records; restart_corun: the classify pass
  // changes its length, the co-run balance is found again.  order: position -> local box of its
  // plan (n_boxes of them); cell_bytes: the rank's f64 cells; slot_free: an observation slot is free.
  struct Decision {
    int mode;
    bool restart_corun;
  };
  Decision decide(const int32_t* order, int n_boxes, double cell_bytes, bool slot_free) {
    Decision decision{0, false};
    if (state == kActive && ++recent_frames >= 32) {
      // repairs in more than half of the frames: the cells change what is visible faster than
      // the observations follow (a repair redoes the tiles that met an unclassified box)
      if (recent_repairs * 2 > recent_frames) {
        state = kBackoff;
        asleep_until = frame + next_backoff;
        next_backoff = std::min(next_backoff * 2, 4096);
        decision.restart_corun = true;  // (the classify pass is the whole pass again)
      } else if (recent_repairs == 0) {
        next_backoff = 64;
      }
      recent_repairs = recent_frames = 0;
    }
    if ((state == kRejected || state == kBackoff) && frame >= asleep_until) {
      state = kObserving;
      std::fill(last_sampled.begin(), last_sampled.end(), int64_t{-1});  // (look afresh)
    }
    // this frame's set: the boxes sampled within the last kSpecMemory frames, in its layer order
    if (state == kObserving || state == kActive) {
      positions.clear();
      flags.assign(flag_bytes(n_boxes), 0);
      bool any_observation = false;
      for (int position = 0; position < n_boxes; ++position) {
        const int64_t last = last_sampled[static_cast<size_t>(order[position])];
        any_observation = any_observation || last >= 0;
        if (last >= 0 && last + kSpecMemory >= frame) {
          positions.push_back(position);
          flags[static_cast<size_t>(position)] = 1;
        }
      }
      if (any_observation) {
        sampled_fraction = static_cast<float>(positions.size()) / static_cast<float>(std::max(n_boxes, 1));
        // Worth it when the part of the classify pass it removes outweighs what it adds (two
        // gated launches and two memsets on the march's stream, ~20 us, and a march that holds a
        // wave per SIMD less): the rank's cells at ~5 TB/s, the unsampled share of that -- at
        // least kSpecMinSavingMs.  (config-4 opaque 0.39 ms saved: frame 0.63 -> 0.43; config-3
        // opaque 0.14, config-2 0.06: 1-2 % SLOWER when tried, their frames are march-bound.)
        const double saving_ms = (1.0 - sampled_fraction) * cell_bytes / 5.0e9;
        const bool worth = sampled_fraction <= worth_it && !positions.empty() && saving_ms >= min_saving_ms;
        if (state == kObserving && worth) {
          state = kActive;
          recent_repairs = recent_frames = 0;
          decision.restart_corun = true;  // (a classify pass of a fraction of the boxes: another balance)
        } else if (state == kObserving) {
          state = kRejected;
          asleep_until = frame + kSpecProbeEvery;
        } else if (!worth) {  // (kActive: the rays reach nearly everything now)
          state = kRejected;
          asleep_until = frame + kSpecProbeEvery;
          decision.restart_corun = true;
        }
      }
    }
    if (state == kActive) {
      decision.mode = 2;
    } else if (state == kObserving && slot_free) {
      decision.mode = 1;
      state = kDeciding;  // (until this observation has arrived)
    }
    return decision;
  }

  // Whether the frame's march records what it samples.  A speculating frame is observed -- a
  // memset, a copy kernel and an event more on the march's stream -- every time while the camera
  // moves or a repair was needed lately: what comes into view is then in the set two or three
  // frames later; every kSpecObserveEvery-th time while the plan stands.  Sparser for a moving
  // camera was tried: a fly-through gains 7 %, sixteen cameras in turn lose 4 % -- the ones that
  // fall between the observations are repaired on every visit.
  bool observed(int mode, bool slot_free, const void* plan) const {
    return mode != 0 && slot_free &&
           (mode == 1 || plan != previous_plan || frame % kSpecObserveEvery == 0 ||
            frame - last_repair < 2 * kSpecObserveEvery);
  }
};

#endif  // AVR_SPECULATION_H
