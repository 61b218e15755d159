/*
 * mgl_owner.h -- one owner for device resources (host code of mgl_api.hip).
 *
 * Every device allocation, pinned-host allocation, event and stream made through a DevOwner is recorded in it and released
 * by its destructor, newest first.  A pointer that merely aliases an allocation is not recorded and so is never freed twice.
 * The handle holds one owner for its whole life; an API call's temporaries hold a local one.  The device the resources live
 * on must be current when the owner dies (mgl_sa_destroy sets it; a call's temporaries die inside the call).
 */
#ifndef MGL_OWNER_H
#define MGL_OWNER_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>

struct DevOwner {
	enum Kind : uint8_t { DEVICE, PINNED, EVENT, STREAM };
	struct Res { void* p; size_t bytes; Kind kind; };
	std::vector<Res> res;
	uint64_t live = 0, live_bytes = 0; /* device allocations held, and their bytes as requested (mgl_debug_dump selector 87) */

	DevOwner() = default;
	DevOwner(const DevOwner&) = delete;
	DevOwner& operator=(const DevOwner&) = delete;
	~DevOwner() { while (!res.empty()) { drop(res.back()); res.pop_back(); } }

	hipError_t device(void** p, size_t bytes)
	{
		const hipError_t e = hipMalloc(p, bytes);
		if (e == hipSuccess) { keep(*p, bytes, DEVICE); live++; live_bytes += bytes; }
		return e;
	}
	hipError_t pinned(void** p, size_t bytes)
	{
		const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
		if (e == hipSuccess) keep(*p, bytes, PINNED);
		return e;
	}
	hipError_t event(hipEvent_t* ev, unsigned flags = hipEventDefault)
	{
		const hipError_t e = hipEventCreateWithFlags(ev, flags);
		if (e == hipSuccess) keep(*ev, 0, EVENT);
		return e;
	}
	hipError_t stream(hipStream_t* s)
	{
		const hipError_t e = hipStreamCreate(s);
		if (e == hipSuccess) keep(*s, 0, STREAM);
		return e;
	}
	/* free one resource ahead of the owner's end (null, or not this owner's: nothing happens) */
	void release(void* p)
	{
		for (size_t i = res.size(); p && i-- > 0;)
			if (res[i].p == p) { drop(res[i]); res.erase(res.begin() + (ptrdiff_t)i); return; }
	}

private:
	void keep(void* p, size_t bytes, Kind kind) { res.push_back(Res{ p, bytes, kind }); }
	void drop(const Res& r)
	{
		switch (r.kind) {
		case DEVICE: (void)hipFree(r.p); live--; live_bytes -= r.bytes; break;
		case PINNED: (void)hipHostFree(r.p); break;
		case EVENT: (void)hipEventDestroy((hipEvent_t)r.p); break;
		case STREAM: (void)hipStreamDestroy((hipStream_t)r.p); break;
		}
	}
};

#endif
