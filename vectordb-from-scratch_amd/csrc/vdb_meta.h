// vdb_meta.h -- what the flat index needs to know about a compiled filter mask (vdb_meta.cpp): where it lives and the event
// behind which it is complete; and how a search that groups by a column (vdb_flat_search_batch_distinct) gets at the column.
// Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "vdb_device.h"

struct vdb_meta_table;

struct vdb_meta_mask {
    vdb_meta_table* table = nullptr;
    int device = 0;
    vdbi::DevBuf<uint64_t> d_words;                         // the mask, in the layout of id_mask
    size_t bits = 0;
    // one device block and its pinned host image: [0] the eligible count (uploaded as 0), then the program
    vdbi::DevBuf<char> d_block; vdbi::HostBuf<char> h_block{hipHostMallocDefault};
    vdbi::Event done;                                       // recorded on the table's stream behind the kernel
};

namespace vdbi {

// A column of a table for a search that reads it on the index's stream.  meta_column_check answers before any device work:
// VDB_ERR_INVALID_ARGUMENT for a null table or a slot never written, else the table's device.  meta_column_acquire LOCKS the
// table, uploads its staged writes (the code vdb_meta_compile uses), and orders `waiter` behind them by an event on the table's
// stream; the column cannot move until meta_column_release.  On failure the table is left unlocked.
struct MetaColumn { const int32_t* d_codes = nullptr; size_t len = 0; };
int meta_column_check(vdb_meta_table* t, uint32_t slot, int* device);
int meta_column_acquire(vdb_meta_table* t, uint32_t slot, hipStream_t waiter, MetaColumn* out);
void meta_column_release(vdb_meta_table* t);

}  // namespace vdbi
