// mf_loss_host.hip.h -- host side of the loss (mf_loss.hip.h): the launches of one evaluation and its read-back.
#pragma once

namespace {

// Row sums of one entry set (CSR over the plan's users) into p->row_sse, then the block sums and the total, all on the
// plan's stream.  `order`: optional list of all rows in the order the workgroups take them.
int launch_loss(mf_plan *p, const int *ptr, const int *idx, const double *val, const int *order)
{
	const int nblocks = p->uc > 0 ? (int) (((long long) p->u0 + p->uc - 1) / mf::kLossBlock - p->u0 / mf::kLossBlock + 1) : 0;
	if (!p->row_sse) {   // the three are allocated together; row_sse marks them
		int rc = p->row_sse.alloc((size_t) p->uc);
		if (rc == MF_OK) rc = p->loss_blocks.alloc((size_t) nblocks);
		if (rc == MF_OK) rc = p->loss_total.alloc(1);
		if (rc != MF_OK) {
			p->row_sse.reset();
			return rc;
		}
	}
	if (p->uc > 0) {
		mf::LossArgs a;
		a.nrows = p->uc;
		a.K = p->K;
		a.stride = p->stride;
		a.ldl = p->ldl;
		a.ldr = p->ldr;
		a.ptr = ptr;
		a.idx = idx;
		a.val = val;
		a.L = p->Lbuf[p->cur];
		a.R = p->Rbuf[p->cur];
		a.row_sse = p->row_sse;
		a.rowlist = order;
		const int few = a.nrows < kSweepFewRows ? 1 : 0;
		a.nch = p->loss_nch[few];
		void *args[] = {&a};
		MF_HIP(hipLaunchKernel((const void *) p->loss_fn, dim3(std::min(a.nrows, 1 << 20)), dim3(mf::kWave), args, p->loss_lds[few],
		                       p->stream));
		hipLaunchKernelGGL(mf::loss_block_kernel, dim3(nblocks), dim3(mf::kWave), 0, p->stream, p->row_sse, p->u0, p->uc, nblocks,
		                   p->loss_blocks);
		MF_HIP(hipGetLastError());
	}
	hipLaunchKernelGGL(mf::loss_total_kernel, dim3(1), dim3(mf::kWave), 0, p->stream, p->loss_blocks, nblocks, p->loss_total);
	MF_HIP(hipGetLastError());
	return MF_OK;
}

// One evaluation: launches, the total (and the row sums when asked for) back to the host, complete on return.
int loss_eval(mf_plan *p, int which, mf_loss *out, double *row_sse)
{
	MF_HIP(hipSetDevice(p->device));
	const bool train = which == MF_LOSS_TRAIN;
	const int rc = train ? launch_loss(p, p->csr_ptr, p->csr_idx, p->csr_val, p->side[1].lpt ? p->side[1].short_rows.get() : nullptr)
	                     : launch_loss(p, p->ho_ptr, p->ho_idx, p->ho_val, nullptr);
	if (rc != MF_OK) return rc;
	double sse = 0.0;
	MF_HIP(hipMemcpyAsync(&sse, p->loss_total, sizeof(double), hipMemcpyDeviceToHost, p->stream));
	if (row_sse && p->uc > 0)
		MF_HIP(hipMemcpyAsync(row_sse, p->row_sse, (size_t) p->uc * sizeof(double), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	out->sse = sse;
	out->count = train ? p->nnz : p->ho_nnz;
	return MF_OK;
}

}  // namespace
