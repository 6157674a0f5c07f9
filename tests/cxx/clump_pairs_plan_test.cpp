// The host plan of the pairwise self-energy (csrc/avr_field_plans.h: plan_clump_pairs) as a plain
// C++ program, built with AddressSanitizer and UBSan and without HIP: every refusal message and
// which one wins when several rules are broken, the items of segments of 0, 1, 2, 255, 256, 257,
// 513, 64 * 256 + 1 and 64 * 256 * 8 + 1 members (the last to show the cap of 64 j tiles per item,
// which a row reaches from 505 tiles on), every tile
// pair covered exactly once, the partial ranges contiguous per segment, depth <= N + 64 for every
// segment, and the limits at 2^22 and 2^31 and one past them, from offsets alone.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../amrvolumerenderer_amd/csrc/avr_field_plans.h"

namespace {

void fail(const std::string& what) {
  std::fprintf(stderr, "FAILED: %s\n", what.c_str());
  std::exit(1);
}
void expect(bool condition, const std::string& what) {
  if (!condition) fail(what);
}

template <class F>
void expect_message(const std::string& message, F&& call) {
  try {
    call();
  } catch (const std::invalid_argument& e) {
    expect(message == e.what(), "expected \"" + message + "\", got \"" + e.what() + "\"");
    return;
  }
  fail("expected \"" + message + "\", but the plan was made");
}

const char* kAscend = "offsets must ascend from 0";
const char* kSegment = "a segment holds more than 2^22 members";
const char* kTotal = "the segments hold 2^31 or more members";
const char* kItems = "the segments make 2^26 or more work items";

std::vector<int64_t> offsets_of(const std::vector<int64_t>& counts) {
  std::vector<int64_t> offsets(1, 0);
  for (int64_t c : counts) offsets.push_back(offsets.back() + c);
  return offsets;
}

avr::ClumpPairsPlan plan_of(const std::vector<int64_t>& counts) {
  const std::vector<int64_t> offsets = offsets_of(counts);
  return avr::plan_clump_pairs(offsets.data(), counts.size());
}

// Every rule the items of one plan must keep, against the counts they were planned from.
void check_items(const std::vector<int64_t>& counts, const std::string& name) {
  const std::vector<int64_t> offsets = offsets_of(counts);
  const avr::ClumpPairsPlan plan = avr::plan_clump_pairs(offsets.data(), counts.size());
  expect(plan.partial_begin.size() == counts.size() + 1 && plan.partial_begin[0] == 0,
         name + ": partial_begin");
  expect(plan.depth.size() == counts.size(), name + ": depth size");
  expect(plan.args.n_items == plan.items.size() && plan.partial_begin.back() == plan.items.size(),
         name + ": n_items");
  expect(plan.args.n_segments == counts.size(), name + ": n_segments");
  expect(plan.scratch_bytes == plan.items.size() * sizeof(double), name + ": scratch");
  for (size_t s = 0; s < counts.size(); ++s) {
    const uint32_t n = static_cast<uint32_t>(counts[s]);
    const uint32_t first = plan.partial_begin[s], last = plan.partial_begin[s + 1];
    expect(first <= last, name + ": partial ranges ascend");
    if (n < 2) {
      expect(first == last && plan.depth[s] == 0, name + ": a segment without pairs has no item");
      continue;
    }
    const uint32_t tiles = (n + 255) / 256;
    std::map<std::pair<uint32_t, uint32_t>, int> covered;
    uint32_t most_tiles = 0;
    for (uint32_t at = first; at < last; ++at) {
      const avr::ClumpPairItem& item = plan.items[at];
      expect(item.begin == static_cast<uint32_t>(offsets[s]) && item.count == n,
             name + ": an item's segment");
      const uint32_t j_first = item.j_tiles & 0xffffu, j_count = item.j_tiles >> 16;
      expect(j_count >= 1 && j_count <= 64, name + ": 1 to 64 j tiles per item");
      expect(item.i_tile < tiles && j_first >= item.i_tile && j_first + j_count <= tiles,
             name + ": an item's tiles");
      most_tiles = std::max(most_tiles, j_count);
      for (uint32_t j = j_first; j < j_first + j_count; ++j) ++covered[{item.i_tile, j}];
    }
    expect(covered.size() == static_cast<size_t>(tiles) * (tiles + 1) / 2,
           name + ": every tile pair is covered");
    for (const auto& pair : covered) expect(pair.second == 1, name + ": a tile pair twice");
    // depth: the lane's terms, 8 + 3 for the workgroup, the reduction's strided terms, 6
    const int64_t lane = std::min<int64_t>(n, int64_t{most_tiles} * 256);
    const int64_t strided = (int64_t{last} - first + 63) / 64;
    expect(plan.depth[s] == lane + 8 + 3 + strided + 6, name + ": depth");
    expect(plan.depth[s] <= int64_t{n} + 64, name + ": depth <= N + 64");
  }
}

}  // namespace

int main() {
  // ---- the refusals, and which one wins ---------------------------------------------------------
  expect_message("null argument", [] { avr::plan_clump_pairs(nullptr, 0); });
  {
    const std::vector<int64_t> from_one = {1, 2}, descending = {0, 5, 4}, negative = {0, -1};
    expect_message(kAscend, [&] { avr::plan_clump_pairs(from_one.data(), 1); });
    expect_message(kAscend, [&] { avr::plan_clump_pairs(from_one.data(), 0); });
    expect_message(kAscend, [&] { avr::plan_clump_pairs(descending.data(), 2); });
    expect_message(kAscend, [&] { avr::plan_clump_pairs(negative.data(), 1); });
    // a descent wins over a segment that is too large, and that over the total
    const int64_t big = (int64_t{1} << 22) + 1;
    const std::vector<int64_t> both = {0, big, big - 1};
    expect_message(kAscend, [&] { avr::plan_clump_pairs(both.data(), 2); });
    std::vector<int64_t> many(1, 0);
    for (int s = 0; s < 512; ++s) many.push_back(many.back() + (int64_t{1} << 22));
    many.push_back(many.back() + big);
    expect_message(kSegment, [&] { avr::plan_clump_pairs(many.data(), many.size() - 1); });
  }
  // ---- the limits, from offsets alone ----------------------------------------------------------
  {
    const int64_t most = int64_t{1} << 22;
    const avr::ClumpPairsPlan plan = plan_of({most});
    expect(plan.depth[0] <= most + 64, "2^22: depth");
    expect(plan.items.size() == 64u * (256u * 257u / 2u), "2^22: items");  // 16384 rows, chunks of 64
    expect_message(kSegment, [&] { plan_of({most + 1}); });
    // the member total: offsets written out up to 2^31 - 1 in segments of 2^22 (which the item
    // limit refuses, below), and one member past it, which the total refuses first
    std::vector<int64_t> counts(511, most);
    counts.push_back(most - 1);
    const std::vector<int64_t> offsets = offsets_of(counts);
    expect(offsets.back() == (int64_t{1} << 31) - 1, "the total below the limit");
    std::vector<int64_t> past = offsets;
    past.back() += 1;
    expect_message(kTotal, [&] { avr::plan_clump_pairs(past.data(), counts.size()); });
    // the items are counted before any table is made: 2105344 per segment of 2^22 members, so
    // 31 of them stay below 2^26 and 32 do not; the total of the members wins over the items
    expect(avr::clump_pair_items(static_cast<uint32_t>(most)) == 2105344u, "items of 2^22");
    expect(31u * 2105344u < avr::kClumpPairMaxItems && 32u * 2105344u >= avr::kClumpPairMaxItems,
           "31 segments of 2^22 fit");
    const std::vector<int64_t> thirty_two = offsets_of(std::vector<int64_t>(32, most));
    expect_message(kItems, [&] { avr::plan_clump_pairs(thirty_two.data(), 32); });
    // one member below 2^31 in segments of 2^22: the members pass, the items do not
    expect_message(kItems, [&] { avr::plan_clump_pairs(offsets.data(), counts.size()); });
  }
  // ---- items -----------------------------------------------------------------------------------
  check_items({}, "no segment");
  check_items({0}, "empty");
  check_items({1}, "one member");
  check_items({2}, "two members");
  check_items({255}, "255");
  check_items({256}, "256");
  check_items({257}, "257");
  check_items({513}, "513");
  check_items({4099}, "4099");
  check_items({64 * 256 + 1}, "65 tiles");
  check_items({64 * 256 * 8 + 1}, "past the j-chunk cap");
  check_items({0, 1, 2, 255, 0, 256, 257, 0, 0, 513, 1, 4099, 0}, "mixed");
  {
    std::vector<int64_t> counts;
    for (int64_t n = 0; n <= 1200; ++n) counts.push_back(n);
    check_items(counts, "0 to 1200");
  }
  {  // the chunk: rows of a few tiles are cut finely, rows of many at 64
    expect(avr::clump_pair_chunk(1) == 1 && avr::clump_pair_chunk(8) == 1 &&
               avr::clump_pair_chunk(9) == 2 && avr::clump_pair_chunk(17) == 3 &&
               avr::clump_pair_chunk(512) == 64 && avr::clump_pair_chunk(16384) == 64,
           "clump_pair_chunk");
    const avr::ClumpPairsPlan plan = plan_of({4099});  // 17 tiles in chunks of 3
    expect(plan.items.size() == 57, "4099: several items per row");
    expect(plan.items[0].i_tile == 0 && plan.items[0].j_tiles == (0u | 3u << 16) &&
               plan.items[5].j_tiles == (15u | 2u << 16) && plan.items[6].i_tile == 1 &&
               plan.items[6].j_tiles == (1u | 3u << 16),
           "4099: the first rows' items");
    const avr::ClumpPairsPlan capped = plan_of({64 * 256 * 8 + 1});  // 513 tiles
    expect(capped.items[0].j_tiles == (0u | 64u << 16) && capped.items[8].j_tiles == (512u | 1u << 16),
           "the j-chunk cap");
  }
  {  // visit_tables: the items, then the partial ranges
    const avr::ClumpPairsPlan plan = plan_of({3, 300});
    avr::ClumpPairArgs args = plan.args;
    int order = 0;
    struct Visit {
      const avr::ClumpPairsPlan* plan;
      int* order;
      void operator()(const avr::ClumpPairItem** to, const avr::ClumpPairItem* host, size_t n) {
        expect(*order == 0 && *to == nullptr && host == plan->items.data() && n == 4, "items");
        ++*order;
      }
      void operator()(const uint32_t** to, const uint32_t* host, size_t n) {
        expect(*order == 1 && *to == nullptr && host == plan->partial_begin.data() && n == 3,
               "partial_begin");
        ++*order;
      }
    };
    plan.visit_tables(&args, Visit{&plan, &order});
    expect(order == 2, "visit_tables names two tables");
    expect(plan.partial_begin[1] == 1 && plan.partial_begin[2] == 4, "partial ranges of {3, 300}");
  }
  std::printf("ok\n");
  return 0;
}
