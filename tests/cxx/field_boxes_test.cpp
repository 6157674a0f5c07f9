// CPU check of the box rules of the cell-scan products (amrvolumerenderer_amd/csrc/
// avr_field_boxes.h) and of the tile count against the tile decode (avr_cell_tiles.h).  Cells are
// never dereferenced by the code under test, so made-up addresses stand for them.
//   field_boxes_test      runs all cases, prints "ok", exit code 0
#include <cstdio>
#include <set>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../amrvolumerenderer_amd/csrc/avr_cell_tiles.h"
#include "../../amrvolumerenderer_amd/csrc/avr_field_boxes.h"

namespace {

int failures = 0;
void expect(bool ok, const std::string& what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s\n", what.c_str());
    ++failures;
  }
}

const char* const kLevel = "a box's level is not below n_levels";
const char* const kDiffer = "the scenes' boxes differ in dims or level";
const char* const kNoCells = "box has no cell data";
const char* const kSpan = "box spans more than 2^28 cells (or has negative strides)";
const char* const kTooMany = "scene has too many cells";

const double* address(uintptr_t a) { return reinterpret_cast<const double*>(a); }
const double* const kCells = address(0x10000);  // 16-byte aligned

// a dense box of nx x ny x nz cells
avr_box box(int nx, int ny, int nz, int level = 0, const double* cells = kCells) {
  avr_box b{};
  b.dims[0] = nx;
  b.dims[1] = ny;
  b.dims[2] = nz;
  b.level = level;
  b.cells = cells;
  b.jstride = nx;
  b.kstride = static_cast<int64_t>(nx) * ny;
  return b;
}

// the message a call refuses with; "" if it does not
template <typename F>
std::string refusal(F&& call) {
  try {
    call();
  } catch (const std::invalid_argument& e) {
    return e.what();
  }
  return "";
}

struct Walk {
  bool cells = false;
  int32_t paired = -1;
  std::vector<avr::FieldView> views;
};
Walk walk(const std::vector<avr_box>& fields, size_t reference, int n_levels = 4) {
  std::vector<const avr_box*> in;
  for (const avr_box& f : fields) in.push_back(&f);
  Walk w;
  w.views.resize(fields.size());
  w.cells = avr::field_box_views(fields[reference], in.data(), static_cast<int>(in.size()),
                                 n_levels, w.views.data(), &w.paired);
  return w;
}
std::string walk_refusal(const std::vector<avr_box>& fields, size_t reference = 0, int n_levels = 4) {
  return refusal([&] { walk(fields, reference, n_levels); });
}

void messages() {
  const avr_box good = box(8, 4, 4, 1);
  expect(walk_refusal({good, good, good}) == "", "messages: three equal boxes pass");
  {
    avr_box b = good;
    b.level = 4;
    expect(walk_refusal({b, b}) == kLevel, "messages: level == n_levels");
    b.level = -1;
    expect(walk_refusal({b, b}) == kLevel, "messages: negative level");
    b.level = 3;
    expect(walk_refusal({b, b}) == "", "messages: level n_levels - 1 passes");
  }
  for (int d = 0; d < 3; ++d) {
    avr_box other = good;
    other.dims[d] += 1;
    expect(walk_refusal({good, other}) == kDiffer, "messages: dims differ");
    expect(walk_refusal({good, good, other}) == kDiffer, "messages: dims differ in the third field");
  }
  {
    avr_box other = good;
    other.level = 2;
    expect(walk_refusal({good, other}) == kDiffer, "messages: level differs");
    // derive's order: the inputs, then the output as the reference
    expect(walk_refusal({other, good}, 1) == kDiffer, "messages: an input differs from the output");
  }
  {
    avr_box null_cells = good;
    null_cells.cells = nullptr;
    expect(walk_refusal({good, null_cells}) == kNoCells, "messages: null cells");
    expect(refusal([&] { avr::field_view(null_cells); }) == kNoCells, "messages: null cells, one view");
  }
  {
    avr_box wide = good;
    wide.kstride = int64_t{1} << 28;
    expect(walk_refusal({good, wide}) == kSpan, "messages: span");
    expect(refusal([&] { avr::field_view(wide); }) == kSpan, "messages: span, one view");
  }
  {
    std::vector<uint32_t> prefix(1, 0u);
    expect(refusal([&] { avr::append_tiles(&prefix, UINT32_MAX); }) == kTooMany, "messages: tiles");
  }
}

// for every pair of rules one box can break together, the earlier rule's message
void precedence() {
  const avr_box good = box(8, 4, 4, 1);
  avr_box bad_level = good;
  bad_level.level = 7;
  {
    avr_box other = bad_level;
    other.dims[0] = 9;
    expect(walk_refusal({bad_level, other}) == kLevel, "precedence: level before differing dims");
    other = bad_level;
    other.cells = nullptr;
    expect(walk_refusal({other, other}) == kLevel, "precedence: level before null cells");
    other = bad_level;
    other.jstride = -8;
    expect(walk_refusal({other, other}) == kLevel, "precedence: level before the span");
  }
  {
    avr_box other = good;
    other.dims[1] = 5;
    other.cells = nullptr;
    expect(walk_refusal({good, other}) == kDiffer, "precedence: differing dims before null cells");
    other.cells = kCells;
    other.kstride = int64_t{1} << 28;
    expect(walk_refusal({good, other}) == kDiffer, "precedence: differing dims before the span");
  }
  {
    avr_box other = good;
    other.cells = nullptr;
    other.kstride = int64_t{1} << 28;
    expect(walk_refusal({good, other}) == kNoCells, "precedence: null cells before the span");
    expect(refusal([&] { avr::field_view(other); }) == kNoCells,
           "precedence: null cells before the span, one view");
  }
  {
    // fields in order: the first field's cells before the second field's dims
    avr_box first = good, second = good;
    first.cells = nullptr;
    second.dims[2] = 5;
    expect(walk_refusal({first, second}) == kNoCells, "precedence: field 0's cells before field 1's dims");
    first = good;
    first.jstride = -8;
    expect(walk_refusal({first, second}) == kSpan, "precedence: field 0's span before field 1's dims");
  }
  {
    // an empty box still has to agree with the others
    avr_box empty = box(0, 4, 4, 1, nullptr);
    expect(walk_refusal({empty, good}) == kDiffer, "precedence: an empty box's dims are compared");
    avr_box leveled = empty;
    leveled.level = 2;
    expect(walk_refusal({empty, leveled}) == kDiffer, "precedence: an empty box's level is compared");
    leveled.level = 9;
    expect(walk_refusal({leveled, leveled}) == kLevel, "precedence: an empty box's level is checked");
  }
  {
    // a box past the span limit never reaches the tile count
    avr_box huge = box(1, 1 << 18, 1 << 18);
    std::vector<uint32_t> prefix(1, 0u);
    const std::string message = refusal([&] {
      walk({huge, huge}, 0);
      avr::append_tiles(&prefix, avr::cell_tiles(1, 1 << 18, 1 << 18));
    });
    expect(message == kSpan, "precedence: the span before the tile count");
  }
}

void paired() {
  const avr_box good = box(8, 4, 4);
  for (size_t n_fields = 1; n_fields <= 7; ++n_fields) {
    std::vector<avr_box> fields(n_fields, good);
    Walk w = walk(fields, 0);
    expect(w.cells && w.paired == 1, "paired: aligned cells and even strides");
    for (size_t f = 0; f < n_fields; ++f) {
      expect(w.views[f].cells == kCells && w.views[f].jstride == 8 && w.views[f].kstride == 32 &&
                 w.views[f].last == 7 + 3 * 8 + 3 * 32 && w.views[f].paired,
             "paired: the view holds the box's cells, strides and last cell");
    }
    for (size_t f = 0; f < n_fields; ++f) {
      for (int fault = 0; fault < 3; ++fault) {
        fields.assign(n_fields, good);
        if (fault == 0) fields[f].cells = address(0x10008);
        if (fault == 1) fields[f].jstride = 9;
        if (fault == 2) fields[f].kstride = 33;
        w = walk(fields, n_fields - 1);
        expect(w.cells && w.paired == 0,
               "paired: 0 for field " + std::to_string(f) + " of " + std::to_string(n_fields) +
                   (fault == 0 ? " at +8 bytes" : fault == 1 ? " with an odd jstride" : " with an odd kstride"));
        for (size_t g = 0; g < n_fields; ++g) {
          expect(w.views[g].paired == (g != f), "paired: per view");
        }
      }
    }
  }
}

void empty_boxes() {
  for (int d = 0; d < 3; ++d) {
    avr_box empty = box(8, 4, 4, 2, nullptr);
    empty.dims[d] = 0;
    expect(avr::box_is_empty(empty), "empty: one dim 0");
    std::vector<avr_box> fields(3, empty);
    Walk w;
    w.views.assign(3, avr::FieldView{kCells, 5, 7, 9, true});  // must be cleared
    std::vector<const avr_box*> in = {&fields[0], &fields[1], &fields[2]};
    const std::string message = refusal([&] {
      w.cells = avr::field_box_views(fields[0], in.data(), 3, 4, w.views.data(), &w.paired);
    });
    expect(message == "" && !w.cells, "empty: accepted with null cells, holds no cells");
    expect(w.paired == 1, "empty: paired stays 1");
    for (const avr::FieldView& v : w.views) {
      expect(v.cells == nullptr && v.jstride == 0 && v.kstride == 0 && v.last == 0 && !v.paired,
             "empty: views zeroed");
    }
    std::vector<uint32_t> prefix = {0u, 5u};
    avr::append_tiles(&prefix, w.cells ? avr::cell_tiles(8, 4, 4) : 0u);
    expect(prefix == std::vector<uint32_t>({0u, 5u, 5u}), "empty: adds zero tiles");
  }
  expect(!avr::box_is_empty(box(1, 1, 1)), "empty: a box of one cell is not");
}

void span_limit() {
  const int64_t limit = int64_t{1} << 28;
  {
    avr_box row = box(1 << 28, 1, 1);  // span = nx - 1
    expect(refusal([&] { avr::field_view(row); }) == "" &&
               avr::field_view(row).last == limit - 1, "span: 2^28 - 1 along x passes");
    row.dims[0] += 1;
    expect(refusal([&] { avr::field_view(row); }) == kSpan, "span: 2^28 along x is refused");
  }
  for (int axis = 1; axis <= 2; ++axis) {
    avr_box b = box(1, 1, 1);
    b.dims[axis] = 2;
    (axis == 1 ? b.jstride : b.kstride) = limit - 1;
    expect(walk_refusal({b, b}) == "" && walk({b, b}, 0).views[1].last == limit - 1,
           "span: 2^28 - 1 by a stride passes");
    (axis == 1 ? b.jstride : b.kstride) = limit;
    expect(walk_refusal({b, b}) == kSpan, "span: 2^28 by a stride is refused");
  }
  {
    // all three terms together: 127 + 3 * 128 + 1 * kstride
    avr_box b = box(128, 4, 2);
    b.jstride = 128;
    b.kstride = limit - 1 - 127 - 3 * 128;
    expect(walk_refusal({b}) == "" && walk({b}, 0).views[0].last == limit - 1, "span: the sum at 2^28 - 1");
    b.kstride += 1;
    expect(walk_refusal({b}) == kSpan, "span: the sum at 2^28");
  }
  {
    avr_box b = box(8, 4, 4);
    b.jstride = -8;
    expect(walk_refusal({b}) == kSpan, "span: a negative jstride");
    b = box(8, 4, 4);
    b.kstride = -32;
    expect(walk_refusal({b}) == kSpan, "span: a negative kstride");
    // ... also where the stride is never applied
    b = box(8, 1, 1);
    b.jstride = -1;
    expect(walk_refusal({b}) == kSpan, "span: a negative jstride of a single row");
    b = box(8, 1, 1);
    b.kstride = -1;
    expect(refusal([&] { avr::field_view(b); }) == kSpan, "span: a negative kstride of a single plane");
  }
}

void prefix() {
  {
    // one box whose own tiles are past 31 bits (strides 0: the span rule is not what refuses it)
    avr_box b = box(1, 1 << 18, 1 << 18);
    b.jstride = b.kstride = 0;
    expect(walk_refusal({b, b}) == "", "prefix: the box itself passes the walk");
    expect(avr::cell_tiles(1, 1 << 18, 1 << 18) == UINT32_MAX, "prefix: 2^32 tiles count as UINT32_MAX");
    std::vector<uint32_t> prefix(1, 0u);
    expect(refusal([&] { avr::append_tiles(&prefix, avr::cell_tiles(1, 1 << 18, 1 << 18)); }) == kTooMany &&
               prefix.size() == 1, "prefix: a box of (1, 2^18, 2^18) is refused");
  }
  const uint32_t half = avr::cell_tiles(1, 1 << 17, 1 << 17);
  // (2^15 - 1) x (2^15 + 1) bricks
  const uint32_t less = avr::cell_tiles(1, 4 * ((1 << 15) - 1), 4 * ((1 << 15) + 1));
  expect(half == (1u << 30) && less == (1u << 30) - 1, "prefix: boxes of 2^30 and 2^30 - 1 tiles");
  {
    std::vector<uint32_t> prefix(1, 0u);
    avr::append_tiles(&prefix, half);
    expect(refusal([&] { avr::append_tiles(&prefix, half); }) == kTooMany, "prefix: a sum of 2^31 is refused");
    expect(prefix == std::vector<uint32_t>({0u, 1u << 30}), "prefix: a refusal appends nothing");
    avr::append_tiles(&prefix, less);
    expect(prefix == std::vector<uint32_t>({0u, 1u << 30, (1u << 31) - 1}), "prefix: a sum of 2^31 - 1 passes");
    avr::append_tiles(&prefix, 0u);
    expect(prefix.back() == (1u << 31) - 1, "prefix: an empty box after it passes");
    expect(refusal([&] { avr::append_tiles(&prefix, 1u); }) == kTooMany, "prefix: one more tile is refused");
  }
}

// cell_tile_of over [0, cell_tiles) yields every (chunk, bj, bk) of the box once, none outside it
void count_and_decode() {
  for (int nx : {1, 127, 128, 129, 300}) {
    for (int ny = 1; ny <= 9; ++ny) {
      for (int nz = 1; nz <= 9; ++nz) {
        const int chunks = (nx + 127) / 128, bricks_y = (ny + 3) / 4, bricks_z = (nz + 3) / 4;
        const uint32_t tiles = avr::cell_tiles(nx, ny, nz);
        const std::string where = " at " + std::to_string(nx) + " x " + std::to_string(ny) + " x " +
                                  std::to_string(nz);
        expect(tiles == static_cast<uint32_t>(chunks * bricks_y * bricks_z), "decode: the count" + where);
        std::set<std::tuple<int, int, int>> seen;
        bool inside = true;
        for (uint32_t local = 0; local < tiles; ++local) {
          const avr::CellTile t = avr::cell_tile_of(nx, ny, local);
          inside = inside && t.chunk >= 0 && t.chunk < chunks && t.bj >= 0 && t.bj < bricks_y &&
                   t.bk >= 0 && t.bk < bricks_z;
          // a tile inside the box holds at least one of its cells
          inside = inside && t.chunk * 128 < nx && t.bj * 4 < ny && t.bk * 4 < nz;
          seen.insert(std::make_tuple(t.chunk, t.bj, t.bk));
        }
        expect(inside, "decode: no tile outside the box" + where);
        expect(seen.size() == tiles, "decode: every tile exactly once" + where);
      }
    }
  }
}

}  // namespace

int main() {
  messages();
  precedence();
  paired();
  empty_boxes();
  span_limit();
  prefix();
  count_and_decode();
  if (failures == 0) std::puts("ok");
  return failures == 0 ? 0 : 1;
}
