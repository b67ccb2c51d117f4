// Where a sequence of a padded batch ends, for a conv-as-GEMM loader, an epilogue or a kernel: the policy of every
// stage that takes exact lengths (FaCodec decode, facodec.hip; PVA flow's graph of launches, durgen.hip; the loaders of
// gemm.hpp).  The dense form is empty and answers the batch stride; the exact form reads the utterance's own length.
#pragma once

namespace fl {

// end(b, n): the end of utterance b at a stage whose batch stride is n rows.  Work that exists only for exact lengths
// sits behind `if constexpr (End::kExact)`, so a dense instantiation is the code it was without the policy.
template <bool EX>
struct SeqEnd {
  static constexpr bool kExact = EX;
  static SeqEnd make(const int*, int) { return {}; }
  __device__ int end(int, int n) const { return n; }
};
template <>
struct SeqEnd<true> {
  static constexpr bool kExact = true;
  const int* __restrict__ lens;  // B device ints (handle-owned, filled stream-ordered per call)
  int mul;                       // rows per length unit at this stage (the decoder's upsampling so far)
  static SeqEnd make(const int* lens, int mul) { return {lens, mul}; }
  // no clamp to [0, n] here: every entry point checks 1 <= lens[b] <= its n on the host before the upload, and the
  // loaders evaluate this per chunk and per stored element
  __device__ int end(int b, int) const { return lens[b] * mul; }
};

}  // namespace fl
