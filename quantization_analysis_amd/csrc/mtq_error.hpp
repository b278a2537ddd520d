// mtq_error.hpp — thread-local error reporting shared by the translation units of libmtq_hip.so.
#pragma once
#include "../../include/mtq.h"

namespace mtq {
// Records `msg` as the calling thread's last error and returns `code`.
int fail(int code, const char *msg);
int failf(int code, const char *fmt, ...);
// MTQ_OK when a HIP device is usable by this process, MTQ_ERR_NO_DEVICE otherwise (cached).
int require_device();
// Zeroed device counters for one K1 launch (persistent waves claim their units from them): kWorkGroups counters,
// kWorkStride unsigneds apart.  Slots come from a per-device ring of kWorkSlots; the follow-up kernel of the launch
// (tile_stats_redo_flagged) sets the slot back to zero, so no memset sits on the stream.  A slot is handed out again only
// behind the event recorded after that follow-up kernel (mtq_slot_ring.hpp): more than kWorkSlots pending launches queue
// instead of sharing counters.
constexpr int kWorkGroups = 64, kWorkStride = 32, kWorkSlots = 128;
// Word 1 of a slot carries the id of the last launch that marked a tile for the literal fix-up (ids are unique per launch,
// so the word never needs resetting): the follow-up kernel returns at once unless it finds its own launch's id there.
constexpr int kWorkStamp = 1;
// Word 2 of a slot counts the waves of the launch that have finished (exact-integer bf16 kernel): the wave that completes the count sets
// the unit counters and this word back to zero, so that launch needs no follow-up kernel for the reset (round 3).
constexpr int kWorkDone = 2;
// Grid of a K1 launch over `total` units (bf16 kernel) or tiles (direct kernel), the ONE place its arithmetic lives (both launchers
// and mtq_debug_k1_grid call it).  Waves claim units from the group counters above: group g of `groups` = min(blocks, kWorkGroups)
// owns units g, g + groups, …  Three regimes:
//   all resident        every unit has a wave of its own and the blocks fit the chip (need <= max_blocks): quota 0;
//   quota, resident     waves retire after `quota` claims, and the grid that needs is still no larger than max_blocks;
//   oversubscribed      the units need more blocks at `quota` per wave than are resident at once: whole counter groups plus one
//                       spare block per group (a block that finds its group's queue empty exits at once).
// quota 0 on input: waves never retire (a fully persistent grid of at most max_blocks).
struct K1Grid { int64_t blocks; int quota, groups; };
inline K1Grid k1_grid(int64_t total, int cus, int waves_per_simd, int waves_per_block, int quota)
{
    const int64_t need = (total + waves_per_block - 1) / waves_per_block;
    const int64_t max_blocks = (int64_t)cus * waves_per_simd * 4 / waves_per_block;   // resident blocks: that many waves on each of a CU's 4 SIMDs
    K1Grid g{need < max_blocks ? need : max_blocks, 0, 0};
    if (quota > 0 && need > max_blocks) {
        const int64_t by_quota = (total + (int64_t)waves_per_block * quota - 1) / ((int64_t)waves_per_block * quota);
        g.blocks = ((by_quota + kWorkGroups - 1) / kWorkGroups + 1) * kWorkGroups;
        if (g.blocks < max_blocks) g.blocks = max_blocks;
        g.quota = quota;
    }
    g.groups = (int)(g.blocks < kWorkGroups ? g.blocks : kWorkGroups);
    return g;
}
// MTQ_K1_UNITS_PER_WAVE, read once (default 8; 0 or negative: persistent waves).  The direct kernel's quota is 16 tiles per unit of it.
int k1_units_per_wave();
// The direct kernel's share of mtq_debug_k1_grid (mtq_direct.hip): waves per block, waves per SIMD, tiles of quota per unit of the switch.
void direct_k1_constants(int *waves_per_block, int *waves_per_simd, int *quota_scale);
unsigned next_launch_id();
struct WorkSlot { unsigned *counters = nullptr; int index = -1, device = -1; };
// MTQ_OK and a slot whose previous user `stream` now waits for, or MTQ_ERR_HIP.
int work_counter_acquire(void *stream, WorkSlot *out);
// Records the slot's event on `stream` (behind the follow-up kernel) and gives the slot back.
void work_counter_release(const WorkSlot &slot, void *stream);
// The launch the slot was acquired for could not be enqueued: the slot goes back without a new event.
void work_counter_abandon(const WorkSlot &slot);
// hipGetLastError() → MTQ_OK / MTQ_ERR_HIP with the kernel name in the message.
int check_launch(const char *what);
// mtq_quantize for MTQ_FMT_MXFP4 / MTQ_FMT_NVFP4, arguments already checked (mtq_fp4_proxy.hip)
int fp4_proxy_quantize(const void *x, int in_dtype, int64_t rows, int64_t cols, int64_t ld, int fmt, float *y, int64_t ldy, void *stream);
// mtq_shutdown's parts (each translation unit releases what it owns; none of them runs from a static destructor)
void scan_shutdown();       // mtq_scan.hip: the device jump-ahead tables
void host_shutdown();       // mtq_host.cpp: the scan thread pool
} // namespace mtq
