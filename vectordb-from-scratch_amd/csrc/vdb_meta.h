// vdb_meta.h -- what the flat index needs to know about a compiled filter mask (vdb_meta.cpp): where it lives and the event
// behind which it is complete.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct vdb_meta_table;

struct vdb_meta_mask {
    vdb_meta_table* table = nullptr;
    int device = 0;
    uint64_t* d_words = nullptr; size_t cap_words = 0;     // the mask, in the layout of id_mask
    size_t bits = 0;
    // one device block and its pinned host image: [0] the eligible count (uploaded as 0), then the program
    char* d_block = nullptr; char* h_block = nullptr;
    hipEvent_t done = nullptr;                              // recorded on the table's stream behind the kernel
};
