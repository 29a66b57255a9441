// ElfReaderQueues, shared by its two translation units: record_host.cpp (the host queues and elfrq_draw) and rq_device.hip (the
// device mirror and elfrq_dev_draw).  Host types only: nothing here needs the GPU runtime.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <deque>
#include <random>
#include <vector>

#include "../../include/elf_amd.h"

// elf::shared::ReaderQueuesT<Record> (elf/distributed/shared_reader.h:165-340): num_reader queues, each a deque bounded by queue_max_size (ReaderQueueT::Insert :88-100),
// filled by TrainCtrl::OnReceive with InsertWithParity(record, rng, reward > 0) (train/game_ctrl.h:306-311; shared_reader.h:212-219):
// games Black won go to the odd queues, the others to the even ones.  A record here is a handle (a slot of an ElfReplay store).
struct ElfReaderQueues {
  struct Rec { int32_t slot, num_moves; };
  std::vector<std::deque<Rec>> qs;
  size_t queue_min_size = 1, queue_max_size = 1000;
  int parity_sizes[2] = {0, 0};
  bool min_size_satisfied = false;
  std::mt19937 insert_rng;                 // TrainCtrl::rng_ (game_ctrl.h:244,367)
  std::vector<std::mt19937> thread_rng;    // GoGameBase::_rng of every GoGameTrain game thread (common/game_base.h:32-38)
  int64_t next_act = 0;                    // acts go round the threads

  // The device mirror's bookkeeping, touched only while a device handle is attached (elfrq_dev_create .. elfrq_dev_destroy).
  // The mirror keeps queue i as a ring of queue_max_size records: deque element j lives at ring position
  // (ring_head[i] + j) % queue_max_size, and a push into a full ring overwrites the front and advances the head.
  struct Touched { int32_t queue, pos; };
  ElfRqDevice* dev = nullptr;
  std::vector<int32_t> ring_head;          // per queue: the ring position of the deque's front
  std::vector<Touched> pending;            // ring positions written since the mirror was last brought up to date
  bool pending_all = false;                // more were written than the rings hold: the next update sends every record
  bool mirror_stale = false;               // an insert happened since the last update
};

// elfrq_insert's note for the mirror, after its push_back (and pop_front if `dropped`) on queue idx.  Only the position is noted:
// the update reads the record that is there when it runs, so a position noted twice is sent twice with the same bytes.
inline void rq_note_insert(ElfReaderQueues* q, int idx, bool dropped) {
  const int32_t qmax = (int32_t)q->queue_max_size, head = q->ring_head[(size_t)idx];
  const int32_t pos = dropped ? head : (int32_t)((head + (int64_t)q->qs[(size_t)idx].size() - 1) % qmax);
  if (dropped) q->ring_head[(size_t)idx] = (head + 1) % qmax;
  q->mirror_stale = true;
  if (q->pending_all) return;
  if (q->pending.size() >= q->qs.size() * q->queue_max_size) { q->pending_all = true; q->pending.clear(); return; }
  q->pending.push_back({(int32_t)idx, pos});
}
