// standin.h -- what the replay program asks of the stand-in runtime (standin.cpp): the ledger of runtime calls since the last take,
// a switch that fails an allocation, and the allocation balance.
#pragma once
#include <stddef.h>

#include <string>

struct dim3_t { unsigned x, y, z; };     // laid out and passed as the runtime's dim3

// every runtime call since the last take, as " name[:detail...]" words in call order
std::string standin_take_ledger();
// the next n allocations fail
void standin_fail_alloc(long n);
void standin_balance(long *allocs, long *frees, long *live);
