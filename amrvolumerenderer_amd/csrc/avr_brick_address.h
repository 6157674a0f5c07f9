// The bricklet byte offset of a cell in four vector instructions, for boxes whose y and z bricklet
// counts are powers of two (kPow2Bricks, avr_internal.h; the layout itself is bricklet_offset's in
// avr_kernels.hip and does not change).  With by = ceil(ny/4) = 2^b and bz = ceil(nz/4) = 2^c the
// two pitches are powers of two and the offset is a set of disjoint bit fields:
//   off = (i&7) | (j&3)<<3 | k<<5 | (j>>2)<<sy | (i>>3)<<sx,   sy = 7 + c,  sx = sy + b
// One 24-bit multiply puts both fields of an index where they belong, with junk between them,
//   t1 = i * (1 + 2^(sx-3))   i&7 at bits 0..2, i>>3 from bit sx on
//   t2 = j * (8 + 2^(sy-2))   j&3 at bits 3..4, j>>2 from bit sy on
// and two bit-field inserts pick the fields out over Z = int(32 * qz) = k<<5 | five bits of the
// fraction, which the inserts overwrite: the z term costs nothing once the factor 32 is folded into
// the constants of the z quotient (an exact power-of-two scaling).
// Plain integer code without HIP on the host, the same four operations as instructions on the
// device: one definition of the form and of its conditions for the march, the host plan and
// tests/cxx/pow2_brick_address_test.cpp, which holds it against bricklet_offset's formula.
#ifndef AVR_BRICK_ADDRESS_H
#define AVR_BRICK_ADDRESS_H

#include <cstdint>

#ifndef AVR_HD  // avr_internal.h's, for a file that includes this header alone
#if defined(__HIP__)
#define AVR_HD __host__ __device__
#else
#define AVR_HD
#endif
#endif

namespace avr {

// log2(v) if v is a power of two, else -1
AVR_HD inline int exact_log2(uint64_t v) {
  if (v == 0 || (v & (v - 1)) != 0) return -1;
  int n = 0;
  while ((v >> n) != 1) ++n;
  return n;
}

// Whether an nx x ny x nz box takes the four-instruction offset, and then its two shifts.
//   by, bz powers of two          the pitches are single bits
//   nx <= 2^(sx-3)                the two copies of i in t1 do not overlap
//   ny <= 2^(sy-5)                nor those of j in t2 (and k<<5 stays below bit sy: nz <= 4 bz)
//   sx - 3 <= 23, sy - 2 <= 23    the multipliers are 24-bit operands (and so are i and j)
//   ceil(nx/8) * 2^sx <= 2^32     the offset itself fits 32 bits: what a product loses above is 0
AVR_HD inline bool pow2_brick_shifts(int nx, int ny, int nz, int* sx_out, int* sy_out) {
  if (nx <= 0 || ny <= 0 || nz <= 0) return false;
  const int b = exact_log2((static_cast<uint64_t>(ny) + 3u) >> 2);
  const int c = exact_log2((static_cast<uint64_t>(nz) + 3u) >> 2);
  if (b < 0 || c < 0) return false;
  const int sy = 7 + c, sx = sy + b;
  if (sx - 3 > 23 || sy - 2 > 23) return false;
  if (static_cast<uint64_t>(nx) > (uint64_t{1} << (sx - 3))) return false;
  if (static_cast<uint64_t>(ny) > (uint64_t{1} << (sy - 5))) return false;
  if ((((static_cast<uint64_t>(nx) + 7u) >> 3) << sx) > (uint64_t{1} << 32)) return false;
  *sx_out = sx;
  *sy_out = sy;
  return true;
}

// The four wave-uniform operands of the form (scalar registers in the march).
struct Pow2BrickKeys {
  uint32_t mul_x, mul_y;    // 1 + 2^(sx-3), 8 + 2^(sy-2)
  uint32_t mask_x, mask_y;  // 7 | ~(2^sx - 1), 0x18 | (2^sx - 2^sy)
};
AVR_HD inline Pow2BrickKeys pow2_brick_keys(int sx, int sy) {
  Pow2BrickKeys keys;
  keys.mul_x = 1u + (1u << (sx - 3));
  keys.mul_y = 8u + (1u << (sy - 2));
  keys.mask_x = 7u | ~((1u << sx) - 1u);
  keys.mask_y = 0x18u | ((1u << sx) - (1u << sy));
  return keys;
}

// v_mul_u32_u24: the low 32 bits of the product of the operands' low 24 bits
AVR_HD inline __attribute__((always_inline)) uint32_t mul_u24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t d;
  asm("v_mul_u32_u24 %0, %1, %2" : "=v"(d) : "s"(b), "v"(a));
  return d;
#else
  return (a & 0xffffffu) * (b & 0xffffffu);
#endif
}
// v_bfi_b32: the bits of `insert` where `mask` is set, those of `base` elsewhere
AVR_HD inline __attribute__((always_inline)) uint32_t bit_insert(uint32_t mask, uint32_t insert,
                                                                 uint32_t base) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t d;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "s"(mask), "v"(insert), "v"(base));
  return d;
#else
  return (insert & mask) | (base & ~mask);
#endif
}

// Byte offset of cell (i, j, z32 >> 5) for 0 <= i < nx, 0 <= j < ny and 0 <= z32 < 32 * nz;
// `keys` must be wave-uniform on the device.
AVR_HD inline __attribute__((always_inline)) uint32_t pow2_brick_offset(uint32_t i, uint32_t j,
                                                                        uint32_t z32,
                                                                        const Pow2BrickKeys& keys) {
  const uint32_t t1 = mul_u24(i, keys.mul_x);
  const uint32_t t2 = mul_u24(j, keys.mul_y);
  return bit_insert(keys.mask_x, t1, bit_insert(keys.mask_y, t2, z32));
}

}  // namespace avr

#endif
