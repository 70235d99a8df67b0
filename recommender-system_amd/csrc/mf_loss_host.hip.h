// mf_loss_host.hip.h -- host side of the loss (mf_loss.hip.h): the launches of one evaluation and its read-back.
#pragma once

namespace {

// blocks of kLossBlock rows, cut at global multiples, that `rows` rows from global row `begin` touch
int blocks_touched(int begin, int rows)
{
	return rows > 0 ? (int) (((long long) begin + rows - 1) / mf::kLossBlock - begin / mf::kLossBlock + 1) : 0;
}

// the row sums, block sums and total of an evaluation, allocated on first use
int loss_buffers(mf_plan *p)
{
	if (p->row_sse) return MF_OK;   // the three are allocated together; row_sse marks them
	int rc = p->row_sse.alloc((size_t) p->uc);
	if (rc == MF_OK) rc = p->loss_blocks.alloc((size_t) blocks_touched(p->u0, p->uc));
	if (rc == MF_OK) rc = p->loss_total.alloc(1);
	if (rc != MF_OK) p->row_sse.reset();
	return rc;
}

// Row sums of one entry set (CSR over the plan's users) into p->row_sse, then the block sums and the total, all on the
// plan's stream.  `order`: optional list of all rows in the order the workgroups take them.  `wgt`: the entries' weights
// (the training set of a weighted plan: q_n * w_n, in the weighted twin of the row-sum kernel) or null.
int launch_loss(mf_plan *p, const int *ptr, const int *idx, const double *val, const int *order, const double *wgt = nullptr)
{
	const int nblocks = blocks_touched(p->u0, p->uc);
	MF_TRY(loss_buffers(p));
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
		a.wgt = wgt;
		const int few = a.nrows < kSweepFewRows ? 1 : 0;
		a.nch = p->loss_nch[few];
		void *args[] = {&a};
		MF_HIP(hipLaunchKernel((const void *) p->loss_fn[wgt != nullptr], dim3(std::min(a.nrows, 1 << 20)), dim3(mf::kWave), args, p->loss_lds[few],
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
	const int rc = train ? launch_loss(p, p->csr_ptr, p->csr_idx, p->csr_val, p->side[1].lpt ? p->side[1].short_rows.get() : nullptr, p->csr_wgt)
	                     : launch_loss(p, p->ho_ptr, p->ho_idx, p->ho_val, nullptr);   // the held-out set stays unweighted
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

// The weights of a weighted plan added up: row sums per user in entry order, then step 4 of the loss, in the loss's
// buffers; the total (and the row sums when asked for) back to the host, complete on return.
int weight_total_eval(mf_plan *p, double *sum_w, double *row_w)
{
	MF_HIP(hipSetDevice(p->device));
	const int nblocks = blocks_touched(p->u0, p->uc);
	MF_TRY(loss_buffers(p));
	if (p->uc > 0) {
		hipLaunchKernelGGL(mf::weight_rows_kernel, dim3(std::min(p->uc, 1 << 20)), dim3(mf::kWave), 0, p->stream, p->csr_ptr.get(),
		                   p->csr_wgt.get(), p->uc, p->row_sse.get());
		MF_HIP(hipGetLastError());
		hipLaunchKernelGGL(mf::loss_block_kernel, dim3(nblocks), dim3(mf::kWave), 0, p->stream, p->row_sse, p->u0, p->uc, nblocks,
		                   p->loss_blocks);
		MF_HIP(hipGetLastError());
	}
	hipLaunchKernelGGL(mf::loss_total_kernel, dim3(1), dim3(mf::kWave), 0, p->stream, p->loss_blocks, nblocks, p->loss_total);
	MF_HIP(hipGetLastError());
	double total = 0.0;
	MF_HIP(hipMemcpyAsync(&total, p->loss_total, sizeof(double), hipMemcpyDeviceToHost, p->stream));
	if (row_w && p->uc > 0) MF_HIP(hipMemcpyAsync(row_w, p->row_sse, (size_t) p->uc * sizeof(double), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	if (sum_w) *sum_w = total;
	return MF_OK;
}

// The implicit-feedback objective of the current factors (mf_plan_implicit_objective): the two Grams (mf_gram.hip.h) and
// their elementwise product summed on the host (mf_backend_gram_dot), the observed part as row sums in the loss's buffers
// followed by step 4 of the loss; complete on return.
constexpr int kImplicitChunk = 32;   // entries per chunk of implicit_rows_kernel: 32 rows of K | 1 doubles, 33 KiB at K = 128

int implicit_objective_eval(mf_plan *p, mf_implicit_objective *out)
{
	MF_HIP(hipSetDevice(p->device));
	MF_TRY(gram_buffers(p));
	MF_TRY(loss_buffers(p));
	MF_TRY(launch_gram(p, 0, 0));
	MF_TRY(launch_gram(p, 1, 0));
	const int nblocks = blocks_touched(p->u0, p->uc);
	if (p->uc > 0) {
		mf::LossArgs a;
		a.nrows = p->uc;
		a.K = p->K;
		a.nch = kImplicitChunk;
		a.stride = p->stride;
		a.ldl = p->ldl;
		a.ldr = p->ldr;
		a.ptr = p->csr_ptr;
		a.idx = p->csr_idx;
		a.val = p->csr_val;
		a.L = p->Lbuf[p->cur];
		a.R = p->Rbuf[p->cur];
		a.row_sse = p->row_sse;
		a.rowlist = p->side[1].lpt ? p->side[1].short_rows.get() : nullptr;
		a.wgt = p->weighted ? p->csr_wgt.get() : nullptr;
		const size_t lds = (size_t) kImplicitChunk * p->stride * sizeof(double);
		hipLaunchKernelGGL(mf::implicit_rows_kernel, dim3(std::min(a.nrows, 1 << 20)), dim3(mf::kWave), lds, p->stream, a, p->confidence);
		MF_HIP(hipGetLastError());
		hipLaunchKernelGGL(mf::loss_block_kernel, dim3(nblocks), dim3(mf::kWave), 0, p->stream, p->row_sse, p->u0, p->uc, nblocks,
		                   p->loss_blocks);
		MF_HIP(hipGetLastError());
	}
	hipLaunchKernelGGL(mf::loss_total_kernel, dim3(1), dim3(mf::kWave), 0, p->stream, p->loss_blocks, nblocks, p->loss_total);
	MF_HIP(hipGetLastError());
	const size_t tri = (size_t) mf::als_triangle(p->K);
	std::vector<double> S;
	try {
		S.resize(2 * tri);
	} catch (const std::bad_alloc &) {
		return MF_ERR_NO_MEMORY;
	}
	double observed = 0.0;
	MF_HIP(hipMemcpyAsync(S.data(), p->gram.get(), 2 * tri * sizeof(double), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipMemcpyAsync(&observed, p->loss_total, sizeof(double), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	out->observed = observed;
	out->count = p->nnz;
	return mf_backend_gram_dot(S.data() + tri, S.data(), p->K, &out->all_sq);   // users' triangle, items' triangle
}

// The penalty of one factor: row sums of squares into `rows_out`, block sums (blocks cut at global multiples of
// kLossBlock counted from `begin`) into `blocks_out`, the total into `total_out`, all on the plan's stream.
int launch_penalty_side(mf_plan *p, const double *X, int begin, int rows, int ld, double *rows_out, double *blocks_out, double *total_out)
{
	const int nblocks = blocks_touched(begin, rows);
	if (rows > 0) {
		hipLaunchKernelGGL(mf::penalty_rows_kernel, dim3((rows + mf::kPenRows - 1) / mf::kPenRows), dim3(mf::kWave), 0, p->stream, X, rows,
		                   p->K, ld, rows_out);
		MF_HIP(hipGetLastError());
		hipLaunchKernelGGL(mf::loss_block_kernel, dim3(nblocks), dim3(mf::kWave), 0, p->stream, rows_out, begin, rows, nblocks, blocks_out);
		MF_HIP(hipGetLastError());
	}
	hipLaunchKernelGGL(mf::loss_total_kernel, dim3(1), dim3(mf::kWave), 0, p->stream, blocks_out, nblocks, total_out);
	MF_HIP(hipGetLastError());
	return MF_OK;
}

// ||L_block||^2 and ||R||^2 of the current factors: launches and read-back, complete on return.
int penalty_eval(mf_plan *p, double *users_sq, double *items_sq, double *user_rows, double *item_rows)
{
	MF_HIP(hipSetDevice(p->device));
	const int nbu = blocks_touched(p->u0, p->uc), nbi = blocks_touched(0, p->items);
	if (!p->pen_total) {   // the three are allocated together; pen_total marks them
		int rc = p->pen_rows.alloc((size_t) p->uc + (size_t) p->items);
		if (rc == MF_OK) rc = p->pen_blocks.alloc((size_t) nbu + (size_t) nbi);
		if (rc == MF_OK) rc = p->pen_total.alloc(2);
		if (rc != MF_OK) {
			p->pen_total.reset();
			return rc;
		}
	}
	double *rows_u = p->pen_rows, *rows_i = rows_u + p->uc;
	double *blocks_u = p->pen_blocks, *blocks_i = blocks_u + nbu;
	double *total = p->pen_total;
	MF_TRY(launch_penalty_side(p, p->Lbuf[p->cur], p->u0, p->uc, p->ldl, rows_u, blocks_u, total));
	MF_TRY(launch_penalty_side(p, p->Rbuf[p->cur], 0, p->items, p->ldr, rows_i, blocks_i, total + 1));
	double t[2] = {0.0, 0.0};
	MF_HIP(hipMemcpyAsync(t, total, sizeof t, hipMemcpyDeviceToHost, p->stream));
	if (user_rows && p->uc > 0) MF_HIP(hipMemcpyAsync(user_rows, rows_u, (size_t) p->uc * sizeof(double), hipMemcpyDeviceToHost, p->stream));
	if (item_rows && p->items > 0) MF_HIP(hipMemcpyAsync(item_rows, rows_i, (size_t) p->items * sizeof(double), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	if (users_sq) *users_sq = t[0];
	if (items_sq) *items_sq = t[1];
	return MF_OK;
}

}  // namespace
