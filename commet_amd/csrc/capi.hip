// capi.hip — implementation of include/commet_hip.h on HIP (gfx950).
// Host side: context (filter slots, scratch of the bucketed index build), HBM
// residency of read sets, pinned multi-threaded ingest, exact chunk planning
// (read_iter.hpp) and the chunk loop of index_and_search on resident sets
// (chunks taken in groups, see search_group_kernel in kernels.hpp).
#include "../../include/commet_hip.h"

#include "kernels.hpp"
#include "index_part.hpp"
#include "slice_search.hpp"
#include "tile_search.hpp"
#include "long_search.hpp"
#include "hit_profile.hpp"
#include "hit_profile_group.hpp"
#include "relative_search.hpp"
#include "hit_profile_jobs.hpp"
#include "hit_profile_wide.hpp"
#include "hit_profile_sliced.hpp"
#include "hit_profile_tiled.hpp"
#include "hits_tags.hpp"
#include "read_filter.hpp"
#include "filter_bits.hpp"
#include "read_iter.hpp"
#include "host/fasta_source.hpp"
#include "host/ingest_pack.hpp"
#include "host/filter_rule.hpp"
#include "host/devmem.hpp"

#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <future>
#include <thread>
#include <string>
#include <vector>

// The implementation, part by part (one translation unit: the kernels above are templates and inline device code, and the
// dispatch-coverage test resolves every launched entry point against this library's own symbol table).
#include "capi/state.hpp"            // errors, launch bookkeeping, commet_ctx, commet_readset
#include "capi/cache.hpp"            // query-list cache, allocations under pressure, scatter workspaces
#include "capi/context.hpp"          // commet_create / _destroy
#include "capi/readset.hpp"          // resident read sets, host ingest
#include "capi/images.hpp"           // packed images, HIP IPC hand-over
#include "capi/residency.hpp"        // commet_readset_offload / _restore: a resident set leaves HBM and comes back
#include "capi/filter.hpp"           // commet_readset_filter: length / N / Shannon / -m on a resident set
#include "capi/index_dispatch.hpp"   // index construction: which path, its launches
#include "capi/search_dispatch.hpp"  // search regimes: which one, its launches
#include "capi/job_parts.hpp"        // what the two job entry points share: phase clock, timing recorder, device planner, pass steps
#include "capi/job.hpp"              // commet_index_reads / _search_reads / _index_and_search
#include "capi/many.hpp"             // what the two many-job calls share: their record, plans, pass packing, the build of a pass's filters
#include "capi/multi.hpp"            // commet_index_many_and_search: several jobs on one search set, their filters in one pass
#include "capi/thresholds.hpp"       // what a profile call leaves of its byte arrays: bytes, or tags and per-file counts (hits_tags_kernel); commet_hits_to_tags
#include "capi/profile.hpp"          // commet_index_and_profile: per-read hit counts, the tags of every t from one job
#include "capi/relative.hpp"         // commet_index_and_search_relative: a threshold per read, a share of the k-mers it can hold
#include "capi/multi_profile.hpp"    // commet_index_many_and_profile: several profile jobs on one search set, their filters in one hits pass
#include "capi/options.hpp"          // commet_set_option, measurement hooks
#include "capi/microbench.hpp"       // commet_membench / _ldsbench
