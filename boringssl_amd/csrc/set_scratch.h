// set_scratch.h -- the layout of a set call's scratch block (dtls_set_api.cc,
// quic_set_api.cc): one block, carved into typed arrays in declaration order.
// A layout states its arrays once, in carve(); the block's size and the
// arrays' places both come from that one list (carve_block runs it twice: over
// no block to measure, then over the block), so they cannot drift apart.
// Arrays are declared by descending alignment, so that nothing is padded.
// Plain C++: no HIP here (tests/test_set_scratch_layout.py carves with malloc).
#ifndef BSSL_AMD_SET_SCRATCH_H
#define BSSL_AMD_SET_SCRATCH_H

#include <stddef.h>
#include <stdint.h>

namespace bssl_amd {

class Carver {
 public:
  // base: the block, aligned to the largest alignment asked for, or null to
  // measure.
  explicit Carver(void *base) : base_(static_cast<uint8_t *>(base)) {}
  // The next n elements of T (null when measuring).
  template <class T>
  T *take(size_t n, size_t align = alignof(T)) {
    used_ = (used_ + align - 1) / align * align;
    T *p = base_ ? reinterpret_cast<T *>(base_ + used_) : nullptr;
    used_ += n * sizeof(T);
    return p;
  }
  size_t size() const { return used_; }

 private:
  uint8_t *base_;
  size_t used_ = 0;
};

// One block from alloc(bytes) (null: failure) carved by l->carve().  Returns
// the block, whose size is left in *bytes, or null.
template <class Layout, class Alloc>
void *carve_block(Layout *l, Alloc &&alloc, size_t *bytes) {
  Carver measure(nullptr);
  l->carve(measure);
  *bytes = measure.size();
  void *block = alloc(*bytes);
  if (!block) return nullptr;
  Carver c(block);
  l->carve(c);
  return block;
}

// BSSL_AMD_DTLS_SET.  Per record: the fragment length (DTLS 1.3 seal), the
// sequence number and the AD length (open), the key index, the run, the nonce,
// the AD, the flag, a status byte and a type byte for a caller who passes
// none; per run: who won, and for an open the run's maximum and its slot's old
// window; the flag word; for an open the index table and the workgroup maxima
// (SetRuns, DtlsSetWindow).  zeroed .. + zeroed_bytes: what a call clears
// first, the flag word and the runs' maxima.
struct DtlsSetLayout {
  uint64_t n, runs, wruns, nb, table_slots = 0;
  uint32_t ad_stride;
  uint64_t *frag_len, *seqs, *ad_len, *zeroed, *run_max, *old, *block_s;
  uint32_t *flag, *key_index, *run_of, *run_won, *block_r, *table;
  uint8_t *nonce, *ad, *valid, *status, *types;
  uint64_t zeroed_bytes;
  DtlsSetLayout(uint64_t records, uint64_t num_runs, uint32_t ad, bool open)
      : n(records), runs(num_runs), wruns(open ? num_runs : 0), nb(open ? (records + 255) / 256 : 0),
        ad_stride(ad) {
    if (open)
      for (table_slots = 512; table_slots < 2 * n;) table_slots *= 2;
  }
  void carve(Carver &c) {
    frag_len = c.take<uint64_t>(n);
    seqs = c.take<uint64_t>(n);
    ad_len = c.take<uint64_t>(n);
    zeroed = c.take<uint64_t>(1);  // the flag word
    flag = reinterpret_cast<uint32_t *>(zeroed);
    run_max = c.take<uint64_t>(wruns);
    zeroed_bytes = 8 * (1 + wruns);
    old = c.take<uint64_t>(6 * wruns);
    block_s = c.take<uint64_t>(nb);
    key_index = c.take<uint32_t>(n);
    run_of = c.take<uint32_t>(n);
    run_won = c.take<uint32_t>(runs);
    block_r = c.take<uint32_t>(nb);
    table = c.take<uint32_t>(table_slots);
    nonce = c.take<uint8_t>(12 * n);
    ad = c.take<uint8_t>(ad_stride * n);
    valid = c.take<uint8_t>(n);
    status = c.take<uint8_t>(n);
    types = c.take<uint8_t>(n);
  }
};

// BSSL_AMD_QUIC_SET.  Per packet: the body's offset and length, the header
// length, the packet number (open), the tag (16-byte aligned), the key index,
// the run, the nonce, the flag and a status byte for a caller who passes none;
// per run: who won; the flag word (SetRuns).  zeroed .. + zeroed_bytes: what a
// call clears first, the flag word.
struct QuicSetLayout {
  uint64_t n, runs;
  uint64_t *body_off, *body_len, *ad_len, *pns, *zeroed;
  uint32_t *flag, *key_index, *run_of, *run_won;
  uint8_t *tags, *nonce, *valid, *status;
  uint64_t zeroed_bytes = 8;
  QuicSetLayout(uint64_t packets, uint64_t num_runs) : n(packets), runs(num_runs) {}
  void carve(Carver &c) {
    body_off = c.take<uint64_t>(n);
    body_len = c.take<uint64_t>(n);
    ad_len = c.take<uint64_t>(n);
    pns = c.take<uint64_t>(n);
    tags = c.take<uint8_t>(16 * n, 16);  // (32 n bytes in)
    zeroed = c.take<uint64_t>(1);        // the flag word
    flag = reinterpret_cast<uint32_t *>(zeroed);
    key_index = c.take<uint32_t>(n);
    run_of = c.take<uint32_t>(n);
    run_won = c.take<uint32_t>(runs);
    nonce = c.take<uint8_t>(12 * n);
    valid = c.take<uint8_t>(n);
    status = c.take<uint8_t>(n);
  }
};

}  // namespace bssl_amd

#endif
