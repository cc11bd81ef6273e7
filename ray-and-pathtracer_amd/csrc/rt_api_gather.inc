// Several contexts in one process (rapt::Renderer::UseDevices): rt_gather_begin / rt_gather_rows, device-to-device pushes of accumulator rows;
// rt_gather_stats_rows, the same with the statistics' rows; rt_gather_active, the listed pixels alone (k_push_active, rt_gather.h).
// Included by rt_api.hip.
int rt_device_of(const rt_ctx* c) { return c ? c->device : -1; }

int rt_gather_begin(rt_ctx* dst)
{
	if (!dst) return RT_E_ARG;
	HIPCHK(dst, hipSetDevice(dst->device));
	if (!dst->rowsFree) HIPCHK(dst, hipEventCreateWithFlags(&dst->rowsFree, hipEventDisableTiming));
	HIPCHK(dst, hipEventRecord(dst->rowsFree, dst->stream));
	return RT_OK;
}

// What the three pushes share.  Every error is reported on SRC -- rt_last_error(src) -- : the call may come from the source context's
// host thread while another thread drives dst, whose error string must not be written from here.
struct Gather {
	rt_ctx *dst, *src;
	const char* what; // the entry point, for the messages

	int check_pair() const
	{
		if (!dst || !src) return fail(src, RT_E_ARG, "%s: null context", what);
		if (dst->width != src->width || dst->height != src->height) return fail(src, RT_E_ARG, "%s: contexts differ in size (%dx%d vs %dx%d)", what, dst->width, dst->height, src->width, src->height);
		return RT_OK;
	}
	int check_rows(int row_first, int row_stride, int row_count) const
	{
		if (!row_set_ok(dst, row_first, row_stride, row_count))
			return fail(src, RT_E_ARG, "%s: rows %d + k*%d (k < %d) outside 0..%d", what, row_first, row_stride, row_count, dst->height);
		return RT_OK;
	}
	// A PUSH on the source's stream: the copy follows the source's rendering in stream order (no host wait), every source
	// context pushes over its own link to the destination at the same time (xGMI is point to point), and the destination's
	// stream waits for the source's event -- what it does next (resolve, the next frame) sees the rows.
	// The push must also come AFTER whatever is already queued on the destination's stream and touches these rows (rt_clear's
	// whole-frame memset on a camera change, the destination's own resolve of the frame before): the source's stream waits for
	// an event recorded on the destination's stream first.  Work queued on dst->stream after this call is ordered by the second event.
	// Which event: the destination's own "rows free" mark of this frame when its owner set one (rt_gather_begin: before dst's share
	// of the frame was queued, so the push waits neither for dst's rendering nor for the sources that pushed earlier -- the pushes
	// overlap, one xGMI link each; ADVICE r5); otherwise one recorded now, behind everything dst's stream holds at this moment.
	// Leaves src's device current.
	int open() const
	{
		if (dst->rowsFree) {
			HIPCHK(src, hipSetDevice(src->device));
			HIPCHK(src, hipStreamWaitEvent(src->stream, dst->rowsFree, 0));
		} else {
			HIPCHK(src, hipSetDevice(dst->device));
			if (!src->gatherReady) HIPCHK(src, hipEventCreateWithFlags(&src->gatherReady, hipEventDisableTiming));
			HIPCHK(src, hipEventRecord(src->gatherReady, dst->stream));
			HIPCHK(src, hipSetDevice(src->device));
			HIPCHK(src, hipStreamWaitEvent(src->stream, src->gatherReady, 0));
		}
		prof_begin(src, K_QUERY); // (with rt_set_profiling on for src: the push's copies or kernel, behind the wait, are one entry of its rt_profile.query)
		return RT_OK;
	}
	// can a copy or a kernel on src's device address dst's memory?  (the same device, or a peer: access is enabled on first use)
	bool direct() const
	{
		if (dst->device == src->device) return true;
		int can = 0;
		bool ok = false;
		if (hipDeviceCanAccessPeer(&can, src->device, dst->device) == hipSuccess && can) {
			const hipError_t e = hipDeviceEnablePeerAccess(dst->device, 0);
			ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
			(void)hipGetLastError();
		}
		return ok;
	}
	// rows row_first + k*row_stride (k < row_count) of one frame-sized array of 'elem'-byte pixels, on src's stream: with peer access one
	// strided copy engine transfer over the link between the two GPUs, else row by row
	int rows(void* to_base, const void* from_base, size_t elem, int row_first, int row_stride, int row_count, bool direct) const
	{
		const size_t rowBytes = (size_t)dst->width * elem, pitch = rowBytes * (size_t)row_stride;
		const char* from = (const char*)from_base + (size_t)row_first * rowBytes;
		char* to = (char*)to_base + (size_t)row_first * rowBytes;
		if (direct) HIPCHK(src, hipMemcpy2DAsync(to, pitch, from, pitch, rowBytes, (size_t)row_count, hipMemcpyDeviceToDevice, src->stream));
		else
			for (int k = 0; k < row_count; k++)
				HIPCHK(src, hipMemcpyPeerAsync(to + (size_t)k * pitch, dst->device, from + (size_t)k * pitch, src->device, rowBytes, src->stream));
		return RT_OK;
	}
	int close() const
	{
		prof_end(src);
		if (!src->gatherDone) HIPCHK(src, hipEventCreateWithFlags(&src->gatherDone, hipEventDisableTiming));
		HIPCHK(src, hipEventRecord(src->gatherDone, src->stream));
		HIPCHK(src, hipSetDevice(dst->device));
		HIPCHK(src, hipStreamWaitEvent(dst->stream, src->gatherDone, 0));
		return RT_OK;
	}
};
#define GATHER_STEP(call) do { const int rc_ = (call); if (rc_ != RT_OK) return rc_; } while (0)

int rt_gather_rows(rt_ctx* dst, rt_ctx* src, int row_first, int row_stride, int row_count)
{
	const Gather G{ dst, src, "rt_gather_rows" };
	GATHER_STEP(G.check_pair());
	GATHER_STEP(G.check_rows(row_first, row_stride, row_count));
	if (dst == src) return RT_OK;
	GATHER_STEP(G.open());
	GATHER_STEP(G.rows(dst->accum, src->accum, sizeof(float4), row_first, row_stride, row_count, G.direct()));
	return G.close();
}

int rt_gather_stats_rows(rt_ctx* dst, rt_ctx* src, int row_first, int row_stride, int row_count)
{
	const Gather G{ dst, src, "rt_gather_stats_rows" };
	GATHER_STEP(G.check_pair());
	GATHER_STEP(G.check_rows(row_first, row_stride, row_count));
	if (!dst->stats.count || !src->stats.count) return fail(src, RT_E_STATE, "rt_gather_stats_rows: statistics are off on the %s context (rt_stats_enable)", src->stats.count ? "destination" : "source");
	if (dst == src) return RT_OK;
	GATHER_STEP(G.open());
	const bool direct = G.direct();
	GATHER_STEP(G.rows(dst->accum, src->accum, sizeof(float4), row_first, row_stride, row_count, direct));
	GATHER_STEP(G.rows(dst->stats.count, src->stats.count, sizeof(uint), row_first, row_stride, row_count, direct));
	GATHER_STEP(G.rows(dst->stats.sumY, src->stats.sumY, sizeof(float), row_first, row_stride, row_count, direct));
	GATHER_STEP(G.rows(dst->stats.sumYY, src->stats.sumYY, sizeof(float), row_first, row_stride, row_count, direct));
	return G.close();
}

int rt_gather_active(rt_ctx* dst, rt_ctx* src)
{
	const Gather G{ dst, src, "rt_gather_active" };
	GATHER_STEP(G.check_pair());
	if (src->nActive < 0) return fail(src, RT_E_STATE, "rt_gather_active: no active-pixel list on the source (rt_select_active, rt_select_budget, their _rows forms, rt_set_active_pixels)");
	if (!dst->stats.count || !src->stats.count) return fail(src, RT_E_STATE, "rt_gather_active: statistics are off on the %s context (rt_stats_enable)", src->stats.count ? "destination" : "source");
	if (dst == src || src->nActive == 0) return RT_OK;
	// the kernel runs on src's device and stores through dst's pointers: they must be addressable from there (asked before anything is queued)
	HIPCHK(src, hipSetDevice(src->device));
	if (!G.direct()) return fail(src, RT_E_UNSUPPORTED, "rt_gather_active: device %d cannot access device %d as a peer (use rt_gather_stats_rows)", src->device, dst->device);
	GATHER_STEP(G.open());
	hipLaunchKernelGGL(k_push_active, dim3((unsigned)((src->nActive + RT_PUSH_BLOCK - 1) / RT_PUSH_BLOCK)), dim3(RT_PUSH_BLOCK), 0, src->stream,
		src->activeList, src->nActive, src->accum, src->stats, dst->accum, dst->stats);
	HIPCHK(src, hipGetLastError());
	return G.close();
}
#undef GATHER_STEP
