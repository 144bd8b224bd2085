// vdb_meta.h -- what the flat index needs to know about a compiled filter mask (vdb_meta.cpp): where it lives and the event
// behind which it is complete.  Not part of the C ABI.
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
