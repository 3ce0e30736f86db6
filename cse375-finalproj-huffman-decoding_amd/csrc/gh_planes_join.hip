// Byte-plane join (gaphuff.h, "byte planes"), included by gh_decode.hip after gh_batch.hip:
// the kernel of gh_planes_join_device, the inverse of gh_planes_split.hip's.  After a decode
// into the batch's own arena the coded planes of every tensor lie at out_off[stream] there and
// the stored planes in the caller's stored arena; the join interleaves them into the tensors.
// No reference counterpart.
//
// The unit, the walk and the lane's share are the split's: 1024 elements of one tensor per
// wave, lane l owns elements [16 l, 16 l + 16): one 16-byte load per plane (1 KiB contiguous
// per instruction), the byte transpose in registers, E 16-byte stores on the tensor side.  A
// destination that is not 16-byte aligned, and the lane that straddles nelem, store byte by
// byte under the scalar rule's bound: exactly nelem * E bytes of a tensor are written.  Arena
// bytes in [n, round_up(n, 16)) are loaded and never stored: the decode does not write them.
//
// When the walk enters a tensor the wave reads the status words of its coded planes' streams;
// a tensor with a flagged plane is skipped by every wave that meets it, and the wave that holds
// its first unit counts it.  No wave waits for another, there is no barrier and no LDS; every
// loop is bounded by counts the host knows.

constexpr int PJ_TB = 256;  // threads per workgroup: four waves
constexpr int PJ_WAVES = PJ_TB / 64;
static_assert(PLANES_UNIT_ELEMS == 64 * PLANES_GROUP, "a unit is one wave of 16-element lanes");

struct PlanesJoinParams {
  const PlanesTensor* desc;    // off[p]: a coded plane's out_off in the batch's arena, a stored plane's stored_off
  const uint32_t* unit0;       // ntensors + 1
  const uint8_t* out;          // the batch's own output arena
  const uint8_t* stored;       // the caller's stored arena
  const unsigned int* status;  // per stream (GH_ST_*), left by the decode
  unsigned int* bad;           // [0] tensors with a flagged plane
  uint32_t ntensors, nunits;
};

// The lane's 16 elements from 4 E dwords: the first `rem` elements are stored.
template <uint32_t E>
__device__ __forceinline__ void planes_tensor_store(uint8_t* dst, uint32_t rem, bool vec, const uint32_t (&w)[4 * E]) {
  if (vec && rem == PLANES_GROUP) {
#pragma unroll
    for (uint32_t j = 0; j < E; ++j) ((uint4*)dst)[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
  } else {
    const uint32_t nb = rem * E;
#pragma unroll
    for (uint32_t d = 0; d < 4 * E; ++d) {
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k)
        if (4 * d + k < nb) dst[4 * d + k] = (uint8_t)(w[d] >> (8 * k));
    }
  }
}

template <uint32_t E>
__device__ __forceinline__ void planes_join_unit(const PlanesJoinParams& p, const PlanesTensor& d, uint32_t blk, int lane) {
  const unsigned long long i0 = (unsigned long long)blk * PLANES_UNIT_ELEMS + (uint32_t)lane * PLANES_GROUP;
  const uint32_t rem = i0 >= d.nelem ? 0u : d.nelem - i0 >= PLANES_GROUP ? PLANES_GROUP : (uint32_t)(d.nelem - i0);
  if (!rem) return;
  const bool vec = (((uintptr_t)d.data) & 15u) == 0;
  uint32_t w[4 * E], pl[E][4];
#pragma unroll
  for (uint32_t q = 0; q < E; ++q) {
    // (inside the plane's extent: both arenas give every plane round_up(nelem, 16) bytes)
    const uint4 v = *(const uint4*)((((d.mask >> q) & 1u) ? p.out : p.stored) + d.off[q] + i0);
    pl[q][0] = v.x;
    pl[q][1] = v.y;
    pl[q][2] = v.z;
    pl[q][3] = v.w;
  }
  planes_join16<E>(pl, w);
  planes_tensor_store<E>(d.data + i0 * E, rem, vec, w);
}

__global__ __launch_bounds__(PJ_TB) void gh_planes_join_kernel(const PlanesJoinParams p) {
  const int lane = threadIdx.x & 63;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t u0, u1;
  unit_run<PJ_WAVES>(p.nunits, wid, u0, u1);
  UnitCursor c;
  PlanesTensor d{};
  bool bad = false;
  for (uint32_t u = u0; u < u1; ++u) {
    if (unit_enter(p.unit0, p.ntensors, u, c)) {
      d = p.desc[c.s];
      unsigned int st = 0;
      for (uint32_t q = 0; q < PLANES_MAX_E; ++q)
        if ((d.mask >> q) & 1u) st |= p.status[d.stream[q]];
      bad = __builtin_amdgcn_readfirstlane((int)st) != 0;
    }
    if (bad) {
      if (c.blk == 0 && lane == 0) atomicAdd(p.bad, 1u);
      continue;
    }
    switch (d.elem) {  // (wave-uniform)
      case 1: planes_join_unit<1>(p, d, c.blk, lane); break;
      case 2: planes_join_unit<2>(p, d, c.blk, lane); break;
      case 4: planes_join_unit<4>(p, d, c.blk, lane); break;
      default: planes_join_unit<8>(p, d, c.blk, lane); break;
    }
  }
}
