// Byte-plane split (gaphuff.h, "byte planes"), included by gh_encode.hip after gh_ebatch.hip:
// the load kernel of gh_planes_load_device.  It stands where gh_ebatch_copy_kernel stands and
// leaves the input arena as that kernel leaves it, for streams that are the coded planes of
// typed tensors; the stored planes go to the caller's stored arena.  No reference counterpart.
//
// The unit of work is PLANES_UNIT_ELEMS = 1024 consecutive elements of one tensor: one wave
// takes E KiB of the tensor and gives 1 KiB to each of its E planes, which is one unit
// (GH_EBATCH_UNIT_BYTES) of every coded plane's stream, so plane unit k is tensor unit k.
// unit0[0 .. ntensors] is the prefix of the tensors' unit counts and the walk is gh_units.hpp's.
// Lane l owns elements [16 l, 16 l + 16) of the unit: E 16-byte loads on the tensor side (the
// wave's E instructions cover the unit's E KiB), the byte transpose in registers by
// gh_planes.hpp's permutes, one 16-byte store per plane (1 KiB contiguous per instruction).
// A tensor whose pointer is not 16-byte aligned, and the lane that straddles nelem, load
// byte by byte under the scalar rule's bound: exactly nelem * E bytes of a tensor are read.
//
// What is written: for a coded plane every byte of the stream's arena extent -- its whole
// units, zero past nelem, and the 32 tail bytes after them (the tensor's last unit); for a
// stored plane [0, round_up(nelem, 16)), zero past nelem.  No wave waits for another, there is
// no barrier and no LDS; every loop is bounded by counts the host knows.

constexpr int PL_TB = 256;  // threads per workgroup: four waves
constexpr int PL_WAVES = PL_TB / 64;
static_assert(PLANES_UNIT_ELEMS == EB_UNIT, "a tensor unit is one unit of every plane's stream");
static_assert(PLANES_UNIT_ELEMS == 64 * PLANES_GROUP, "a unit is one wave of 16-element lanes");
static_assert(EBATCH_TAIL_BYTES == 32, "the tail is two 16-byte stores");

struct PlanesSplitParams {
  const PlanesTensor* desc;  // off[p]: a coded plane's in_off in the input arena, a stored plane's stored_off
  const uint32_t* unit0;     // ntensors + 1
  uint8_t* in;               // the batch's input arena
  uint8_t* stored;           // the caller's stored arena
  uint32_t ntensors, nunits;
};

// The lane's 16 elements as 4 E dwords, zero past `rem` elements.
template <uint32_t E>
__device__ __forceinline__ void planes_tensor_load(const uint8_t* src, uint32_t rem, bool vec, uint32_t (&w)[4 * E]) {
  if (vec && rem == PLANES_GROUP) {
#pragma unroll
    for (uint32_t j = 0; j < E; ++j) {
      const uint4 v = ((const uint4*)src)[j];
      w[4 * j] = v.x;
      w[4 * j + 1] = v.y;
      w[4 * j + 2] = v.z;
      w[4 * j + 3] = v.w;
    }
  } else {
    const uint32_t nb = rem * E;
#pragma unroll
    for (uint32_t d = 0; d < 4 * E; ++d) {
      uint32_t x = 0;
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k)
        if (4 * d + k < nb) x |= (uint32_t)src[4 * d + k] << (8 * k);
      w[d] = x;
    }
  }
}

template <uint32_t E>
__device__ __forceinline__ void planes_split_unit(const PlanesSplitParams& p, const PlanesTensor& d, uint32_t blk,
                                                  bool last, int lane) {
  const unsigned long long i0 = (unsigned long long)blk * PLANES_UNIT_ELEMS + (uint32_t)lane * PLANES_GROUP;
  const uint32_t rem = i0 >= d.nelem ? 0u : d.nelem - i0 >= PLANES_GROUP ? PLANES_GROUP : (uint32_t)(d.nelem - i0);
  const bool vec = (((uintptr_t)d.data) & 15u) == 0;
  uint32_t w[4 * E], pl[E][4];
  planes_tensor_load<E>(d.data + i0 * E, rem, vec, w);
  planes_split16<E>(w, pl);
#pragma unroll
  for (uint32_t q = 0; q < E; ++q) {
    const bool coded = (d.mask >> q) & 1u;
    uint8_t* dst = (coded ? p.in : p.stored) + d.off[q] + i0;
    if (coded || rem) *(uint4*)dst = make_uint4(pl[q][0], pl[q][1], pl[q][2], pl[q][3]);
    // the stream's tail after its last unit
    if (coded && last && lane < 2)
      *(uint4*)(p.in + d.off[q] + ((unsigned long long)blk + 1u) * PLANES_UNIT_ELEMS + 16u * (uint32_t)lane) =
          make_uint4(0u, 0u, 0u, 0u);
  }
}

__global__ __launch_bounds__(PL_TB) void gh_planes_split_kernel(const PlanesSplitParams p) {
  const int lane = threadIdx.x & 63;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t u0, u1;
  unit_run<PL_WAVES>(p.nunits, wid, u0, u1);
  UnitCursor c;
  PlanesTensor d{};
  for (uint32_t u = u0; u < u1; ++u) {
    if (unit_enter(p.unit0, p.ntensors, u, c)) d = p.desc[c.s];
    const bool last = u + 1u == c.end;
    switch (d.elem) {  // (wave-uniform)
      case 1: planes_split_unit<1>(p, d, c.blk, last, lane); break;
      case 2: planes_split_unit<2>(p, d, c.blk, last, lane); break;
      case 4: planes_split_unit<4>(p, d, c.blk, last, lane); break;
      default: planes_split_unit<8>(p, d, c.blk, last, lane); break;
    }
  }
}
