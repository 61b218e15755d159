/*
 * mgl_exchange.inc -- best-slab exchange between chains (SURVEY 8e; main.c:75-77 restarts later epochs
 * from packets_best): part of mgl_api.hip.
 *
 * One chain per GPU / process.  An exchange is the one collective north_star names: a single 8-byte
 * all-reduce(min) of (best_cost << 8 | rank) -- latency-bound -- and then one broadcast of the winner's
 * best slab in its packed 8-byte device form.  mgl_sa_exchange_best holds the protocol (who wins, who
 * adopts); the two collectives go through one of two transports behind the same mgl_comm handle:
 *
 *   RCCL  (mgl_comm_init)      ncclAllReduce(ncclMin, ncclUint64) + ncclBroadcast over xGMI, straight from the
 *                              winner's HBM into the others' (no host hop).  librccl is loaded on first use
 *                              (dlopen), so single-GPU users do not need it; the two enum values the calls pass
 *                              are checked against rccl.h when this file is compiled.
 *   host  (mgl_comm_init_shm)  a shared-memory file: keys and the slab are staged through it.  For chains that
 *                              share one GPU (RCCL refuses two ranks per device) and for boxes without RCCL;
 *                              it is also how the two-rank protocol is tested on a one-GPU box.
 *
 * Two more collectives serve the exchange that crosses every chain's best slab (mgl_sa_exchange_cross_all): an all-gather of
 * one u64 per rank (ncclAllGather; the host form reads the keys the min already stages) and the broadcast again, once per parent.
 *
 * An adopted slab becomes packets_best only; its cost is the sender's exact figure.  It is verified when
 * it is used: mgl_sa_begin_epoch(from_best) re-derives its structures with the parallel builder, checks
 * every packet against the input (k_validate) and the total against the claimed cost.
 */
#include <atomic>
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>
#include <algorithm>
#include <type_traits>
#include <utility>

#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
/* the values passed through the dlsym'ed entry points below are rccl.h's */
#define MGL_NCCL_UINT64 ((int)ncclUint64)
#define MGL_NCCL_MIN ((int)ncclMin)
static_assert((int)ncclUint64 == 5 && (int)ncclMin == 3, "rccl.h: ncclUint64 / ncclMin are not the values this library was written against");
static_assert(sizeof(ncclUniqueId) == 128, "rccl.h: ncclUniqueId is not 128 bytes (mgl_comm_unique_id's contract)");
static_assert(std::is_same<decltype(&ncclAllGather), ncclResult_t (*)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t)>::value,
              "rccl.h: ncclAllGather does not have the signature it is called with");
#else
#error "rccl/rccl.h not found: the RCCL enum values used by mgl_sa_exchange_best cannot be checked"
#endif

/* librccl prints a version banner on stdout when a communicator comes up; stdout is where the compressor
 * writes its stream (main.c:110-119) and where bench.py prints its one JSON line: send anything the library
 * says during set-up to stderr instead */
struct StdoutGuard {
	int saved;
	StdoutGuard() { fflush(stdout); saved = dup(1); if (saved >= 0) dup2(2, 1); }
	~StdoutGuard() { fflush(stdout); if (saved >= 0) { dup2(saved, 1); close(saved); } }
};

struct mgl_nccl_id { char internal[128]; };
typedef int (*pfn_ncclGetUniqueId)(void*);
typedef int (*pfn_ncclCommInitRank)(void**, int, /* ncclUniqueId by value: 128 bytes */ struct mgl_nccl_id, int);
typedef int (*pfn_ncclCommDestroy)(void*);
typedef int (*pfn_ncclAllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*pfn_ncclBroadcast)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*pfn_ncclAllGather)(const void*, void*, size_t, int, void*, hipStream_t);
typedef const char* (*pfn_ncclGetErrorString)(int);

/* the shared-memory transport's file: one page of header, the slab area behind it */
#define MGL_SHM_MAGIC 0x314D4853434C474Dull /* "MGLCSHM1" */
#define MGL_SHM_HDR_BYTES 4096u
struct ShmHdr {
	std::atomic<uint64_t> magic; /* written last by rank 0 */
	uint64_t nonce;
	uint32_t world, pad;
	std::atomic<uint64_t> arrived; /* barrier: arrivals, all generations (monotone: no reset to race with) */
	std::atomic<uint64_t> sense;   /* last generation every rank has reached */
	uint64_t keys[256];
};
static_assert(sizeof(ShmHdr) <= MGL_SHM_HDR_BYTES, "ShmHdr must fit its page");

#define MGL_COMM_RCCL 0
#define MGL_COMM_SHM 1
struct mgl_comm {
	int kind;
	int rank, world, device;
	/* RCCL */
	void* dl;
	void* comm;
	pfn_ncclCommDestroy destroy;
	pfn_ncclAllReduce all_reduce;
	pfn_ncclBroadcast broadcast;
	pfn_ncclAllGather all_gather;
	pfn_ncclGetErrorString errstr;
	/* shared-memory file */
	int fd;
	unsigned char* map;
	size_t map_bytes;
	std::string path;
	uint64_t gen;
	double timeout_s;
};
#define MGL_KEY_NONE ((1ull << 54) - 1ull) /* "no best slab yet": larger than any real cost (costs stay below 2^44) */

static double comm_timeout_s()
{
	const char* e = getenv("MGL_COMM_TIMEOUT_S");
	const double v = e ? atof(e) : 0.0;
	return v > 0.0 ? v : 600.0;
}
static double now_s()
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static void* rccl_open()
{
	void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
	if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
	if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
	return h;
}

extern "C" int mgl_comm_unique_id(uint8_t id_out[128])
{
	if (!id_out) return fail(MGL_EINVAL, "null argument");
	StdoutGuard guard;
	void* h = rccl_open();
	if (!h) return fail(MGL_EDEVICE, std::string("mgl_comm_unique_id: librccl not found: ") + dlerror());
	pfn_ncclGetUniqueId f = (pfn_ncclGetUniqueId)dlsym(h, "ncclGetUniqueId");
	if (!f) return fail(MGL_EDEVICE, "mgl_comm_unique_id: ncclGetUniqueId missing");
	const int rc = f(id_out);
	if (rc != 0) return fail(MGL_EDEVICE, "ncclGetUniqueId failed");
	return MGL_OK;
}

extern "C" int mgl_comm_init(mgl_comm** out, const uint8_t id[128], int rank, int world, int device)
{
	if (!out || !id || world < 1 || rank < 0 || rank >= world || world > 256) return fail(MGL_EINVAL, "mgl_comm_init: bad arguments");
	HIPCHK(hipSetDevice(device));
	StdoutGuard guard;
	mgl_comm* c = new (std::nothrow) mgl_comm();
	if (!c) return fail(MGL_ENOMEM, "out of host memory");
	c->kind = MGL_COMM_RCCL; c->fd = -1;
	c->dl = rccl_open();
	if (!c->dl) { delete c; return fail(MGL_EDEVICE, std::string("mgl_comm_init: librccl not found: ") + dlerror()); }
	pfn_ncclCommInitRank init = (pfn_ncclCommInitRank)dlsym(c->dl, "ncclCommInitRank");
	c->destroy = (pfn_ncclCommDestroy)dlsym(c->dl, "ncclCommDestroy");
	c->all_reduce = (pfn_ncclAllReduce)dlsym(c->dl, "ncclAllReduce");
	c->broadcast = (pfn_ncclBroadcast)dlsym(c->dl, "ncclBroadcast");
	c->all_gather = (pfn_ncclAllGather)dlsym(c->dl, "ncclAllGather");
	c->errstr = (pfn_ncclGetErrorString)dlsym(c->dl, "ncclGetErrorString");
	if (!init || !c->destroy || !c->all_reduce || !c->broadcast || !c->all_gather) { delete c; return fail(MGL_EDEVICE, "mgl_comm_init: RCCL symbols missing"); }
	mgl_nccl_id uid;
	memcpy(uid.internal, id, 128);
	c->rank = rank; c->world = world; c->device = device;
	const int rc = init(&c->comm, world, uid, rank);
	if (rc != 0) {
		const std::string why = c->errstr ? c->errstr(rc) : "?";
		delete c;
		return fail(MGL_EDEVICE, "ncclCommInitRank: " + why);
	}
	*out = c;
	return MGL_OK;
}

/* ---- the host shared-memory transport */
static int shm_remap(mgl_comm* c, size_t need)
{
	if (c->map && c->map_bytes >= need) return MGL_OK;
	struct stat sb;
	if (fstat(c->fd, &sb) != 0) return fail(MGL_EDEVICE, "mgl_comm (shm): fstat failed");
	if ((size_t)sb.st_size < need) return fail(MGL_EDEVICE, "mgl_comm (shm): the file is smaller than the slab it should hold");
	if (c->map) munmap(c->map, c->map_bytes);
	c->map = (unsigned char*)mmap(nullptr, (size_t)sb.st_size, PROT_READ | PROT_WRITE, MAP_SHARED, c->fd, 0);
	if (c->map == MAP_FAILED) { c->map = nullptr; c->map_bytes = 0; return fail(MGL_ENOMEM, "mgl_comm (shm): mmap failed"); }
	c->map_bytes = (size_t)sb.st_size;
	return MGL_OK;
}
static int shm_barrier(mgl_comm* c)
{
	ShmHdr* h = (ShmHdr*)c->map;
	const uint64_t g = ++c->gen;
	const uint64_t a = h->arrived.fetch_add(1, std::memory_order_acq_rel) + 1;
	if (a == g * (uint64_t)c->world) { h->sense.store(g, std::memory_order_release); return MGL_OK; }
	const double t0 = now_s();
	unsigned spins = 0;
	while (h->sense.load(std::memory_order_acquire) < g) {
		if (++spins > 2000) usleep(200);
		if ((spins & 1023u) == 0 && now_s() - t0 > c->timeout_s)
			return fail(MGL_EDEVICE, "mgl_comm (shm): a peer chain did not arrive at the exchange within MGL_COMM_TIMEOUT_S");
	}
	return MGL_OK;
}

extern "C" int mgl_comm_init_shm(mgl_comm** out, const char* path, uint64_t nonce, int rank, int world, int device)
{
	if (!out || !path || !*path || world < 1 || rank < 0 || rank >= world || world > 256) return fail(MGL_EINVAL, "mgl_comm_init_shm: bad arguments");
	mgl_comm* c = new (std::nothrow) mgl_comm();
	if (!c) return fail(MGL_ENOMEM, "out of host memory");
	c->kind = MGL_COMM_SHM; c->rank = rank; c->world = world; c->device = device; c->fd = -1;
	c->path = path; c->timeout_s = comm_timeout_s();
	if (rank == 0) {
		/* a file left by an earlier (crashed) run is not ours: start from a fresh one, published under its final
		 * name only once it is complete (the magic is written last as well) */
		(void)unlink(path);
		c->fd = open(path, O_RDWR | O_CREAT | O_EXCL, 0600);
		if (c->fd < 0 || ftruncate(c->fd, MGL_SHM_HDR_BYTES) != 0) { if (c->fd >= 0) close(c->fd); delete c; return fail(MGL_EDEVICE, std::string("mgl_comm_init_shm: cannot create ") + path); }
		if (shm_remap(c, MGL_SHM_HDR_BYTES) != MGL_OK) { close(c->fd); delete c; return MGL_EDEVICE; }
		ShmHdr* h = (ShmHdr*)c->map;
		h->nonce = nonce; h->world = (uint32_t)world;
		h->arrived.store(0); h->sense.store(0);
		h->magic.store(MGL_SHM_MAGIC, std::memory_order_release);
	} else {
		const double t0 = now_s();
		for (;;) {
			c->fd = open(path, O_RDWR);
			if (c->fd >= 0) {
				struct stat sb;
				if (fstat(c->fd, &sb) == 0 && (size_t)sb.st_size >= MGL_SHM_HDR_BYTES && shm_remap(c, MGL_SHM_HDR_BYTES) == MGL_OK) {
					ShmHdr* h = (ShmHdr*)c->map;
					if (h->magic.load(std::memory_order_acquire) == MGL_SHM_MAGIC && h->nonce == nonce && h->world == (uint32_t)world) break;
					munmap(c->map, c->map_bytes); c->map = nullptr; c->map_bytes = 0;
				}
				close(c->fd); c->fd = -1; /* not there yet, or another run's file (different nonce): look again */
			}
			if (now_s() - t0 > c->timeout_s) {
				delete c;
				return fail(MGL_EDEVICE, std::string("mgl_comm_init_shm: no file of this run (nonce, world) appeared at ") + path + " within MGL_COMM_TIMEOUT_S");
			}
			usleep(20000);
		}
	}
	*out = c;
	const int rc = shm_barrier(c); /* everybody is attached: rank 0 may unlink the name at any time from here on */
	if (rc != MGL_OK) { *out = nullptr; if (c->map) munmap(c->map, c->map_bytes); close(c->fd); if (rank == 0) (void)unlink(path); delete c; return rc; }
	return MGL_OK;
}

extern "C" void mgl_comm_destroy(mgl_comm* c)
{
	if (!c) return;
	if (c->kind == MGL_COMM_RCCL) {
		if (c->comm && c->destroy) (void)c->destroy(c->comm);
	} else {
		if (c->map) munmap(c->map, c->map_bytes);
		if (c->fd >= 0) close(c->fd);
		if (c->rank == 0) (void)unlink(c->path.c_str());
	}
	delete c;
}
extern "C" int mgl_comm_rank(const mgl_comm* c) { return c ? c->rank : -1; }
extern "C" int mgl_comm_world(const mgl_comm* c) { return c ? c->world : 0; }

/* ---- the collectives, by transport */
/* min over the ranks of one u64 each (the packed key): every rank receives it.  `sa` lends a stream and 16 bytes of
 * device scratch to the RCCL form; the host form does not touch the device (sa may be null: mgl_comm_min_u64) */
static int comm_min_u64(mgl_sa* sa, mgl_comm* comm, uint64_t mine, uint64_t* out)
{
	if (comm->kind == MGL_COMM_SHM) {
		ShmHdr* h = (ShmHdr*)comm->map;
		h->keys[comm->rank] = mine;
		int rc = shm_barrier(comm);
		if (rc) return rc;
		uint64_t m = ~0ull;
		for (int r = 0; r < comm->world; r++) m = h->keys[r] < m ? h->keys[r] : m;
		*out = m;
		return shm_barrier(comm); /* nobody writes its next key before everybody has read these */
	}
	if (!sa) return fail(MGL_EINVAL, "an RCCL all-reduce needs a chain (device scratch, stream)");
	uint64_t* d_key = (uint64_t*)sa->d_topk_cost; /* 64 u64 of scratch */
	HIPCHK(hipMemcpyAsync(d_key, &mine, sizeof mine, hipMemcpyHostToDevice, sa->q.stream));
	const int nrc = comm->all_reduce(d_key, d_key + 1, 1, MGL_NCCL_UINT64, MGL_NCCL_MIN, comm->comm, sa->q.stream);
	if (nrc != 0) return fail(MGL_EDEVICE, std::string("ncclAllReduce: ") + (comm->errstr ? comm->errstr(nrc) : "?"));
	HIPCHK(hipMemcpyAsync(out, d_key + 1, sizeof *out, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}
/* one u64 of every rank, in rank order, to every rank (`all`: world entries).  The host form reads every key that comm_min_u64
 * takes the minimum of, between the same two barriers; the RCCL form borrows the chain's stream and allocates world + 1 words for
 * the call (the chain's own scratch holds 64, a communicator up to 256 ranks) */
static int comm_allgather_u64(mgl_sa* sa, mgl_comm* comm, uint64_t mine, uint64_t* all)
{
	if (comm->kind == MGL_COMM_SHM) {
		ShmHdr* h = (ShmHdr*)comm->map;
		h->keys[comm->rank] = mine;
		int rc = shm_barrier(comm);
		if (rc) return rc;
		for (int r = 0; r < comm->world; r++) all[r] = h->keys[r];
		return shm_barrier(comm); /* nobody writes its next word before everybody has read these */
	}
	if (!sa) return fail(MGL_EINVAL, "an RCCL all-gather needs a chain (stream)");
	struct Tmp {
		DevOwner own;
		uint64_t* d = nullptr;
	} tmp;
	TRY(dnew(tmp.own, tmp.d, (size_t)comm->world + 1u));
	HIPCHK(hipMemcpyAsync(tmp.d, &mine, sizeof mine, hipMemcpyHostToDevice, sa->q.stream));
	const int nrc = comm->all_gather(tmp.d, tmp.d + 1, 1, MGL_NCCL_UINT64, comm->comm, sa->q.stream);
	if (nrc != 0) {
		(void)hipStreamSynchronize(sa->q.stream); /* the copy above reads a local and writes what tmp frees */
		return fail(MGL_EDEVICE, std::string("ncclAllGather: ") + (comm->errstr ? comm->errstr(nrc) : "?"));
	}
	HIPCHK(hipMemcpyAsync(all, tmp.d + 1, sizeof(uint64_t) * (size_t)comm->world, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}
/* n packed packets from `send` on the root's device into `recv` on everybody else's */
static int comm_broadcast_slab(mgl_sa* sa, mgl_comm* comm, const mgl_pk* send, mgl_pk* recv, size_t n, int root)
{
	if (comm->kind == MGL_COMM_SHM) {
		const size_t need = (size_t)MGL_SHM_HDR_BYTES + sizeof(mgl_pk) * n;
		int rc;
		if (comm->rank == root) {
			struct stat sb;
			if (fstat(comm->fd, &sb) != 0 || ((size_t)sb.st_size < need && ftruncate(comm->fd, (off_t)need) != 0))
				return fail(MGL_EDEVICE, "mgl_comm (shm): cannot grow the file to hold the slab");
			if ((rc = shm_remap(comm, need)) != MGL_OK) return rc;
			HIPCHK(hipMemcpyAsync(comm->map + MGL_SHM_HDR_BYTES, send, sizeof(mgl_pk) * n, hipMemcpyDeviceToHost, sa->q.stream));
			HIPCHK(hipStreamSynchronize(sa->q.stream));
		}
		if ((rc = shm_barrier(comm)) != MGL_OK) return rc; /* the slab is in the file */
		if (comm->rank != root) {
			if ((rc = shm_remap(comm, need)) != MGL_OK) return rc;
			HIPCHK(hipMemcpyAsync(recv, comm->map + MGL_SHM_HDR_BYTES, sizeof(mgl_pk) * n, hipMemcpyHostToDevice, sa->q.stream));
			HIPCHK(hipStreamSynchronize(sa->q.stream));
		}
		return shm_barrier(comm); /* everybody has its copy: the area may be overwritten */
	}
	const int nrc = comm->broadcast(comm->rank == root ? (const void*)send : (const void*)recv, recv, n, MGL_NCCL_UINT64, root, comm->comm, sa->q.stream);
	if (nrc != 0) return fail(MGL_EDEVICE, std::string("ncclBroadcast: ") + (comm->errstr ? comm->errstr(nrc) : "?"));
	return MGL_OK;
}

/* test hook for the host transport (no device involved): the min of one word per rank */
extern "C" int mgl_comm_min_u64(mgl_comm* comm, uint64_t mine, uint64_t* out)
{
	if (!comm || !out) return fail(MGL_EINVAL, "null argument");
	if (comm->kind != MGL_COMM_SHM) return fail(MGL_EINVAL, "mgl_comm_min_u64: host transport only (the RCCL form needs a chain's stream)");
	return comm_min_u64(nullptr, comm, mine, out);
}

/* the same for the all-gather: every rank's word in rank order (`all_out`: mgl_comm_world entries) */
extern "C" int mgl_comm_allgather_u64(mgl_comm* comm, uint64_t mine, uint64_t* all_out)
{
	if (!comm || !all_out) return fail(MGL_EINVAL, "null argument");
	if (comm->kind != MGL_COMM_SHM) return fail(MGL_EINVAL, "mgl_comm_allgather_u64: host transport only (the RCCL form needs a chain's stream)");
	return comm_allgather_u64(nullptr, comm, mine, all_out);
}

/* the device buffer that holds packets_best right now */
static const mgl_pk* best_slab_device(mgl_sa* sa, const Control& c)
{
	return (sa->incremental && sa->snapshots && c.best_is_current) ? sa->base.v.slab : sa->d_best;
}
/* packets_best := the packed slab at `src` (device), claimed cost `cost` */
static int adopt_best_device(mgl_sa* sa, const mgl_pk* src, uint64_t cost, Control& c)
{
	HIPCHK(hipMemcpyAsync(sa->d_best, src, sizeof(mgl_pk) * (size_t)sa->n, hipMemcpyDeviceToDevice, sa->q.stream));
	if (sa->d_snap_meta) HIPCHK(hipMemsetAsync(sa->d_snap_meta + 1, 0, sizeof(SnapMeta), sa->q.stream));
	c.best_cost = cost;
	c.best_is_current = 0;
	sa->best_unverified = true;
	return write_ctl(sa, sa->base, &c);
}

/* the second half of mgl_sa_exchange_best: the winner's packed slab to everybody, 8 bytes per position (RCCL: HBM to HBM); a rank
 * whose best is dearer, or that has none, adopts it (*adopted, nullable, says so).  `c`: the chain's control block as just read */
static int broadcast_best_and_adopt(mgl_sa* sa, mgl_comm* comm, Control& c, int winner, uint64_t wcost, bool* adopted)
{
	if (adopted) *adopted = false;
	const bool i_win = winner == comm->rank;
	mgl_pk* recv = sa->scratch.v.slab; /* the parity hooks' scratch slab doubles as the landing area */
	int rc;
	if ((rc = comm_broadcast_slab(sa, comm, best_slab_device(sa, c), recv, (size_t)sa->n, winner)) != MGL_OK) return rc;
	if (!i_win && (c.best_cost == 0 || wcost < c.best_cost)) {
		if (adopted) *adopted = true;
		return adopt_best_device(sa, recv, wcost, c);
	}
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}

extern "C" int mgl_sa_exchange_best(mgl_sa* sa, mgl_comm* comm, int* winner_rank, uint64_t* winner_cost)
{
	if (!sa || !comm) return fail(MGL_EINVAL, "null argument");
	if (comm->device != sa->device) return fail(MGL_EINVAL, "mgl_sa_exchange_best: communicator and chain live on different devices");
	HIPCHK(hipSetDevice(sa->device));
	Control c;
	int rc = read_ctl(sa, sa->base, &c);
	if (rc) return rc;
	/* (1) who holds the cheapest slab: one 8-byte all-reduce(min) */
	const uint64_t mine = ((c.best_cost ? c.best_cost : MGL_KEY_NONE) << 8) | (uint64_t)(comm->rank & 0xFF);
	uint64_t key = 0;
	if ((rc = comm_min_u64(sa, comm, mine, &key)) != MGL_OK) return rc;
	const int winner = (int)(key & 0xFF);
	const uint64_t wcost = key >> 8;
	if (winner_rank) *winner_rank = winner;
	if (winner_cost) *winner_cost = wcost == MGL_KEY_NONE ? 0 : wcost;
	if (wcost == MGL_KEY_NONE || comm->world == 1) return MGL_OK; /* nobody has a best slab yet / nobody to send it to */
	/* (2) the winner's packed slab */
	return broadcast_best_and_adopt(sa, comm, c, winner, wcost, nullptr);
}

/* the same hand-over through host memory, for transports other than the library's own (tests use gloo) */
extern "C" int mgl_sa_best_packed(mgl_sa* sa, uint64_t* packed_out, uint64_t* perplexity_out)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	HIPCHK(hipSetDevice(sa->device));
	Control c;
	int rc = read_ctl(sa, sa->base, &c);
	if (rc) return rc;
	if (perplexity_out) *perplexity_out = c.best_cost;
	if (packed_out) {
		HIPCHK(hipMemcpyAsync(packed_out, best_slab_device(sa, c), sizeof(mgl_pk) * (size_t)sa->n, hipMemcpyDeviceToHost, sa->q.stream));
		HIPCHK(hipStreamSynchronize(sa->q.stream));
	}
	return MGL_OK;
}
extern "C" int mgl_sa_adopt_best_packed(mgl_sa* sa, const uint64_t* packed, uint64_t perplexity)
{
	if (!sa || !packed || perplexity == 0) return fail(MGL_EINVAL, "bad argument");
	HIPCHK(hipSetDevice(sa->device));
	Control c;
	int rc = read_ctl(sa, sa->base, &c);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(sa->scratch.v.slab, packed, sizeof(mgl_pk) * (size_t)sa->n, hipMemcpyHostToDevice, sa->q.stream));
	return adopt_best_device(sa, sa->scratch.v.slab, perplexity, c);
}

/* ---- crossing exchange (mgl_crossover.hip): the loser recombines its own best slab with the winner's */
/* packets_best := the packed slab at `src` (device) at its exact cost; `unverified`: checked when an epoch starts from it */
static int xo_set_best(mgl_sa* sa, const mgl_pk* src, uint64_t cost, Control& c, bool unverified)
{
	HIPCHK(hipMemcpyAsync(sa->d_best, src, sizeof(mgl_pk) * (size_t)sa->n, hipMemcpyDeviceToDevice, sa->q.stream));
	if (sa->d_snap_meta) HIPCHK(hipMemsetAsync(sa->d_snap_meta + 1, 0, sizeof(SnapMeta), sa->q.stream));
	c.best_cost = cost;
	c.best_is_current = 0;
	sa->best_unverified = unverified;
	return write_ctl(sa, sa->base, &c);
}
/* mgl_sa_cross_best with `other` already in the scratch slab (an import, or the landing area of a broadcast) */
static int cross_best_scratch(mgl_sa* sa, uint32_t grain, bool from_peer /* or from the caller: not yet compared with the input */, mgl_cross_stats* st)
{
	Control c;
	int rc = read_ctl(sa, sa->base, &c);
	if (rc) return rc;
	const mgl_pk* other = sa->scratch.v.slab;
	memset(st, 0, sizeof *st);
	if (c.best_cost == 0) {
		/* no best slab yet: the walk mgl_sa_set_best uses says what `other` costs */
		Control w;
		HIPCHK(hipMemsetAsync(sa->scratch.ctl, 0, sizeof(Control), sa->q.stream));
		if ((rc = launch_rebuild(sa, sa->scratch, 0, nullptr, nullptr))) return rc;
		if ((rc = read_ctl(sa, sa->scratch, &w))) return rc;
		if (w.error_flags) return fail(MGL_EINVAL, "slab is not a valid parse of the input");
		st->grain = grain ? grain : MGL_XO_DEF_GRAIN;
		st->parent_cost[1] = w.rebuild_cost;
		st->adopted = 1;
		return xo_set_best(sa, other, w.rebuild_cost, c, from_peer);
	}
	XoBufs x;
	if ((rc = xo_alloc(sa, x, 2))) return rc;
	HIPCHK(hipMemcpyAsync(x.slabs, best_slab_device(sa, c), sizeof(mgl_pk) * (size_t)sa->n, hipMemcpyDeviceToDevice, sa->q.stream));
	HIPCHK(hipMemcpyAsync(x.slabs + sa->n, other, sizeof(mgl_pk) * (size_t)sa->n, hipMemcpyDeviceToDevice, sa->q.stream));
	if ((rc = xo_run(sa, x, 2, grain, st))) return rc;
	const uint64_t own = st->parent_cost[0], oth = st->parent_cost[1];
	if (st->child_cost < own && st->child_cost < oth) {
		st->adopted = 2;
		rc = xo_set_best(sa, x.child, st->child_cost, c, from_peer || sa->best_unverified);
	} else if (oth < own) {
		st->adopted = 1;
		rc = xo_set_best(sa, other, oth, c, from_peer);
	}
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize(sa->q.stream)); /* the buffers go away with x */
	return MGL_OK;
}

extern "C" int mgl_sa_cross_best(mgl_sa* sa, const mgl_packet* other, uint32_t grain, mgl_cross_stats* stats)
{
	if (!sa || !other) return fail(MGL_EINVAL, "null argument");
	HIPCHK(hipSetDevice(sa->device));
	int rc = import_slab(sa, other, sa->scratch.v.slab);
	if (rc) return rc;
	mgl_cross_stats st;
	if ((rc = cross_best_scratch(sa, grain, true, &st))) return rc; /* `other` is as little checked as a peer's slab */
	if (stats) *stats = st;
	return MGL_OK;
}

extern "C" int mgl_sa_exchange_cross(mgl_sa* sa, mgl_comm* comm, uint32_t grain, int* winner_rank, uint64_t* winner_cost, mgl_cross_stats* stats)
{
	if (!sa || !comm) return fail(MGL_EINVAL, "null argument");
	if (comm->device != sa->device) return fail(MGL_EINVAL, "mgl_sa_exchange_cross: communicator and chain live on different devices");
	HIPCHK(hipSetDevice(sa->device));
	if (stats) memset(stats, 0, sizeof *stats);
	Control c;
	int rc = read_ctl(sa, sa->base, &c);
	if (rc) return rc;
	/* the two collectives of mgl_sa_exchange_best */
	const uint64_t mine = ((c.best_cost ? c.best_cost : MGL_KEY_NONE) << 8) | (uint64_t)(comm->rank & 0xFF);
	uint64_t key = 0;
	if ((rc = comm_min_u64(sa, comm, mine, &key)) != MGL_OK) return rc;
	const int winner = (int)(key & 0xFF);
	const uint64_t wcost = key >> 8;
	if (winner_rank) *winner_rank = winner;
	if (winner_cost) *winner_cost = wcost == MGL_KEY_NONE ? 0 : wcost;
	if (wcost == MGL_KEY_NONE || comm->world == 1) return MGL_OK;
	if ((rc = comm_broadcast_slab(sa, comm, best_slab_device(sa, c), sa->scratch.v.slab, (size_t)sa->n, winner)) != MGL_OK) return rc;
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	if (winner == comm->rank) return MGL_OK;
	/* every other rank crosses its own best slab with the one that has just landed in the scratch slab */
	mgl_cross_stats st;
	if ((rc = cross_best_scratch(sa, grain, true, &st))) return rc;
	if (stats) *stats = st;
	return MGL_OK;
}

/* ---- crossing exchange of all chains: the parents are the distinct best slabs of every chain, up to MGL_XO_MAX_PARENTS */
/* The selection every rank makes from the same gathered words: the ranks that hold a best slab in ascending key order (cost, then
 * rank), skipping a rank whose (cost, hash) an already selected one has, until MGL_XO_MAX_PARENTS are chosen.  Equal hashes of
 * equal-cost slabs are taken for equal slabs: a collision can only drop a parent, never cross a wrong one in.  Returns D. */
static uint32_t cross_all_select(const uint64_t* keys, const uint64_t* hashes, int world, uint32_t parent_rank[MGL_XO_MAX_PARENTS], uint32_t* with_best)
{
	std::vector<std::pair<uint64_t, uint32_t>> order; /* (key, the rank it came from) */
	for (int r = 0; r < world; r++)
		if ((keys[r] >> 8) != MGL_KEY_NONE) order.push_back(std::make_pair(keys[r], (uint32_t)r));
	std::sort(order.begin(), order.end());
	*with_best = (uint32_t)order.size();
	uint32_t D = 0;
	for (size_t i = 0; i < order.size() && D < MGL_XO_MAX_PARENTS; i++) {
		const uint32_t r = order[i].second;
		bool seen = false;
		for (uint32_t p = 0; p < D && !seen; p++) seen = (keys[parent_rank[p]] >> 8) == (keys[r] >> 8) && hashes[parent_rank[p]] == hashes[r];
		if (!seen) parent_rank[D++] = r;
	}
	return D;
}
/* D >= 2 parents: their owners broadcast them into the slots of the crossover's slab buffer, every rank makes the same child and
 * takes the same decision.  *fell_back: a rank could not allocate the buffers, so nothing was sent and nothing crossed */
static int cross_all_parents(mgl_sa* sa, mgl_comm* comm, Control& c, uint32_t D, const uint32_t* parent_rank, const uint64_t* keys, uint32_t grain,
                             mgl_cross_stats* st, bool* fell_back)
{
	const size_t n = sa->n;
	XoBufs x;
	/* a rank that cannot allocate must not leave the others waiting in a broadcast: everybody learns of it first */
	const uint64_t ok = xo_alloc(sa, x, D) == MGL_OK ? 1u : 0u;
	uint64_t all_ok = 0;
	int rc = comm_min_u64(sa, comm, ok, &all_ok);
	if (rc) return rc;
	*fell_back = all_ok == 0;
	if (*fell_back) return MGL_OK;
	for (uint32_t p = 0; p < D; p++) {
		mgl_pk* slot = x.slabs + (size_t)p * n;
		const int owner = (int)parent_rank[p];
		if (owner == comm->rank) HIPCHK(hipMemcpyAsync(slot, best_slab_device(sa, c), sizeof(mgl_pk) * n, hipMemcpyDeviceToDevice, sa->q.stream));
		if ((rc = comm_broadcast_slab(sa, comm, slot, slot, n, owner)) != MGL_OK) return rc;
	}
	if ((rc = xo_run(sa, x, D, grain, st))) return rc;
	for (uint32_t p = 0; p < D; p++)
		if (st->parent_cost[p] != keys[parent_rank[p]] >> 8)
			return fail(MGL_EINVAL, "mgl_sa_exchange_cross_all: a chain's best slab does not cost what the chain published");
	const uint64_t cheapest = st->parent_cost[0];
	if (st->child_cost < cheapest) {
		st->adopted = 2;
		rc = xo_set_best(sa, x.child, st->child_cost, c, true);
	} else if (c.best_cost == 0 || cheapest < c.best_cost) {
		st->adopted = 1;
		rc = xo_set_best(sa, x.slabs, cheapest, c, true);
	}
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize(sa->q.stream)); /* the buffers go away with x */
	return MGL_OK;
}

extern "C" int mgl_slab_hash(mgl_sa* sa, const mgl_packet* packets, uint64_t* hash)
{
	if (!sa || !hash) return fail(MGL_EINVAL, "null argument");
	HIPCHK(hipSetDevice(sa->device));
	int rc;
	if (packets) {
		if ((rc = import_slab(sa, packets, sa->scratch.v.slab))) return rc;
		return slab_hash_device(sa, sa->scratch.v.slab, hash);
	}
	Control c;
	if ((rc = read_ctl(sa, sa->base, &c))) return rc;
	if (c.best_cost == 0) return fail(MGL_EINVAL, "mgl_slab_hash: the chain has no best slab yet");
	return slab_hash_device(sa, best_slab_device(sa, c), hash);
}

extern "C" int mgl_sa_exchange_cross_all(mgl_sa* sa, mgl_comm* comm, uint32_t grain, mgl_cross_all_stats* stats)
{
	if (!sa || !comm) return fail(MGL_EINVAL, "null argument");
	if (comm->device != sa->device) return fail(MGL_EINVAL, "mgl_sa_exchange_cross_all: communicator and chain live on different devices");
	HIPCHK(hipSetDevice(sa->device));
	mgl_cross_all_stats out;
	memset(&out, 0, sizeof out);
	out.own_parent = UINT32_MAX;
	if (stats) *stats = out;
	Control c;
	int rc = read_ctl(sa, sa->base, &c);
	if (rc) return rc;
	/* (1) publish: the key of mgl_sa_exchange_best and the hash of the best slab, one all-gather each */
	uint64_t hash = 0;
	if (c.best_cost && (rc = slab_hash_device(sa, best_slab_device(sa, c), &hash))) return rc;
	const uint64_t mine = ((c.best_cost ? c.best_cost : MGL_KEY_NONE) << 8) | (uint64_t)(comm->rank & 0xFF);
	std::vector<uint64_t> keys((size_t)comm->world), hashes((size_t)comm->world);
	if ((rc = comm_allgather_u64(sa, comm, mine, keys.data())) != MGL_OK) return rc;
	if ((rc = comm_allgather_u64(sa, comm, hash, hashes.data())) != MGL_OK) return rc;
	/* (2) select: the same parents, in the same order, on every rank */
	const uint32_t D = cross_all_select(keys.data(), hashes.data(), comm->world, out.parent_rank, &out.chains_with_best);
	out.distinct = D;
	for (uint32_t p = 0; p < D; p++)
		if ((int)out.parent_rank[p] == comm->rank) out.own_parent = p;
	/* (3) act */
	bool fell_back = false;
	if (D >= 2) {
		rc = cross_all_parents(sa, comm, c, D, out.parent_rank, keys.data(), grain, &out.cross, &fell_back);
		out.fell_back = fell_back ? 1u : 0u;
	}
	if (rc == MGL_OK && (D == 1 || fell_back) && comm->world > 1) {
		/* one slab is all there is (or all the devices have room for): mgl_sa_exchange_best's broadcast of the cheapest */
		bool adopted = false;
		memset(&out.cross, 0, sizeof out.cross);
		rc = broadcast_best_and_adopt(sa, comm, c, (int)out.parent_rank[0], keys[out.parent_rank[0]] >> 8, &adopted);
		out.cross.adopted = adopted ? 1u : 0u;
	}
	if (D == 1 || fell_back) out.cross.parent_cost[0] = keys[out.parent_rank[0]] >> 8; /* what every chain's best slab costs now */
	if (rc) return rc;
	if (stats) *stats = out;
	return MGL_OK;
}
