// mf_build.hip.h -- CSR/CSC construction (device-side stable radix sort, host fallback) and the row schedule.
#pragma once

namespace {

// Host table -> device, ORDERED WITH THE PLAN'S STREAM.  The plan's stream is created hipStreamNonBlocking: nothing
// orders it with the null stream that a plain hipMemcpy / hipMemset uses, so every set-up transfer goes through the
// plan's own stream and is complete (the host vector may go out of scope) when this returns.  (Round 3: three flaky
// mismatches in the GPU suite, never reproducible alone, all on plans whose set-up mixed the two streams.)
inline hipError_t h2d(mf_plan *p, void *dst, const void *src, size_t bytes)
{
	if (bytes == 0) return hipSuccess;
	const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, p->stream);
	return e != hipSuccess ? e : hipStreamSynchronize(p->stream);
}


// stable counting sort of the entries by `key` into (ptr, idx, val); `wgt` (optional): a second per-entry array that
// travels with val into `w`
void bucket(int64_t nnz, int nkeys, const int32_t *key, int32_t key_off, const int32_t *other,
            int32_t other_off, const double *val, std::vector<int> &ptr, std::vector<int> &idx,
            std::vector<double> &v, std::vector<int> *pos_out = nullptr, const double *wgt = nullptr,
            std::vector<double> *w = nullptr)
{
	if (wgt) w->resize((size_t) nnz);
	if (pos_out) pos_out->resize((size_t) nnz);
	ptr.assign((size_t) nkeys + 1, 0);
	for (int64_t n = 0; n < nnz; ++n) ptr[(size_t) (key[n] - key_off) + 1]++;
	for (int k = 0; k < nkeys; ++k) ptr[(size_t) k + 1] += ptr[k];
	std::vector<int> fill(ptr.begin(), ptr.end() - 1);
	idx.resize((size_t) nnz);
	v.resize((size_t) nnz);
	for (int64_t n = 0; n < nnz; ++n) {
		const int pos = fill[(size_t) (key[n] - key_off)]++;
		idx[(size_t) pos] = other[n] - other_off;
		v[(size_t) pos] = val[n];
		if (wgt) (*w)[(size_t) pos] = wgt[n];
		if (pos_out) (*pos_out)[(size_t) n] = pos;
	}
}


// ---- device-side CSR / CSC build: the entries are uploaded once in file order; a STABLE radix
// sort of a permutation by row (CSR) or by column (CSC) keeps the file order inside every row and column,
// which is what makes the sweeps reproduce the serial summation order.
__global__ void __launch_bounds__(256) prep_keys_kernel(const int *__restrict__ row, const int *__restrict__ col,
                                                        int64_t nnz, int u0, int uc, int items,
                                                        unsigned *__restrict__ rkey, unsigned *__restrict__ perm,
                                                        int *__restrict__ flags)
{
	const int64_t n = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if (n >= nnz) return;
	const int r = row[n] - u0, c = col[n];
	if (r < 0 || r >= uc || c < 0 || c >= items) atomicOr(&flags[0], 1);         // out of range
	if (n > 0 && row[n - 1] > row[n]) atomicOr(&flags[1], 1);                      // not row-sorted
	if (n > 0 && row[n - 1] == row[n] && col[n - 1] > col[n]) atomicOr(&flags[2], 1);   // columns not ascending in a row
	rkey[n] = (unsigned) r;
	perm[n] = (unsigned) n;
}

__global__ void __launch_bounds__(256) gather_kernel(const unsigned *__restrict__ perm, int64_t nnz,
                                                     const int *__restrict__ other, int other_off,
                                                     const double *__restrict__ val, int *__restrict__ idx_out,
                                                     double *__restrict__ val_out, const double *__restrict__ wgt,
                                                     double *__restrict__ wgt_out)
{
	const int64_t n = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if (n >= nnz) return;
	const unsigned s = perm[n];
	idx_out[n] = other[s] - other_off;
	val_out[n] = val[s];
	if (wgt) wgt_out[n] = wgt[s];   // weighted plans: the weight follows its entry through the same permutation
}

// ptr[k] = first position whose (sorted) key is >= k, k = 0..nkeys
__global__ void __launch_bounds__(256) ptr_kernel(const unsigned *__restrict__ sorted, int64_t nnz, int nkeys,
                                                  int *__restrict__ ptr)
{
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k > nkeys) return;
	int64_t lo = 0, hi = nnz;
	while (lo < hi) {
		const int64_t mid = (lo + hi) >> 1;
		if (sorted[mid] < (unsigned) k) lo = mid + 1; else hi = mid;
	}
	ptr[k] = (int) lo;
}

// The band offset table of the user sweep (mf_schedule.h): off[b * nrows + r] = the first entry of row r whose item id is at
// least band b's first item, b = 0 .. bands (blockIdx.y); rows of ascending item ids.  Row 0 of the table is ptr[0 .. nrows)
// and row `bands` is ptr[1 .. nrows].
__global__ void __launch_bounds__(256) band_offsets_kernel(const int *__restrict__ ptr, const int *__restrict__ idx, int nrows, int items,
                                                           int bands, int *__restrict__ off)
{
	const int r = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
	if (r >= nrows || b > bands) return;
	const int beg = ptr[r], end = ptr[r + 1];
	off[(size_t) b * nrows + r] = b == bands ? end : mf_sched::band_cut(idx, beg, end, mf_sched::band_first(b, items, bands));
}

__global__ void __launch_bounds__(256) copy_keys_kernel(const int *__restrict__ src, int64_t nnz,
                                                        unsigned *__restrict__ key, unsigned *__restrict__ perm)
{
	const int64_t n = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if (n >= nnz) return;
	key[n] = (unsigned) src[n];
	perm[n] = (unsigned) n;
}

// inverse of a permutation: inv[perm[q]] = q
__global__ void __launch_bounds__(256) invert_perm_kernel(const unsigned *__restrict__ perm, int64_t nnz,
                                                          int *__restrict__ inv)
{
	const int64_t q = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if (q < nnz) inv[perm[q]] = (int) q;
}

// map[file2csr ? file2csr[perm_csc[q]] : perm_csc[q]] = q: CSR position -> CSC position of the same entry
__global__ void __launch_bounds__(256) csr2csc_kernel(const unsigned *__restrict__ perm_csc, int64_t nnz,
                                                      const int *__restrict__ file2csr, int *__restrict__ map)
{
	const int64_t q = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if (q >= nnz) return;
	const unsigned f = perm_csc[q];
	map[file2csr ? file2csr[f] : (int) f] = (int) q;
}

__global__ void __launch_bounds__(256) fill_records_kernel(const int *__restrict__ idx, int64_t nnz,
                                                           mf::StreamRec *__restrict__ rec)
{
	const int64_t n = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if (n < nnz) rec[n].idx = idx[n];
}

int bits_for(int nkeys)
{
	int b = 1;
	while (b < 32 && (1ll << b) < (long long) nkeys) ++b;
	return b;
}

struct DevTmp {   // frees its buffers on scope exit
	std::vector<dev_buf<char>> bufs;
	template <typename T> int get(T **out, size_t count)
	{
		dev_buf<char> b;
		const int rc = b.alloc(std::max<size_t>(count, 1) * sizeof(T));
		*out = (T *) b.get();
		if (rc == MF_OK) bufs.push_back(std::move(b));
		return rc;
	}
};

// Builds csr_* and csc_* of plan p from host SoA entries.  Returns MF_ERR_ARGUMENT for out-of-range indices.
// the reference's array of structs -> the three arrays the build works on
__global__ void __launch_bounds__(256) split_entries_kernel(const mf_entry *__restrict__ e, int64_t nnz,
                                                            int *__restrict__ row, int *__restrict__ col,
                                                            double *__restrict__ val)
{
	const int64_t n = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if (n >= nnz) return;
	const mf_entry x = e[n];
	row[n] = x.row;
	col[n] = x.col;
	val[n] = x.value;
}

int build_on_device(mf_plan *p, const mf_shard *s, const mf_entry *aos, bool swap, const double *weight, std::vector<int> &csr_ptr_host,
                    std::vector<int> &csc_ptr_host)
{
	const int64_t nnz = s->nnz;
	const size_t nz = (size_t) nnz;
	hipStream_t st = p->stream;
	MF_TRY(p->csr_ptr.alloc((size_t) p->uc + 1));
	MF_TRY(p->csc_ptr.alloc((size_t) p->items + 1));
	MF_TRY(p->csr_idx.alloc(nz + 64));
	MF_TRY(p->csr_val.alloc(nz + 64));
	MF_TRY(p->csc_idx.alloc(nz + 64));
	MF_TRY(p->csc_val.alloc(nz + 64));
	if (weight) {
		MF_TRY(p->csr_wgt.alloc(nz + 64));
		MF_TRY(p->csc_wgt.alloc(nz + 64));
	}
	csr_ptr_host.assign((size_t) p->uc + 1, 0);
	csc_ptr_host.assign((size_t) p->items + 1, 0);
	if (nnz == 0) {
		MF_HIP(hipMemsetAsync(p->csr_ptr, 0, ((size_t) p->uc + 1) * sizeof(int), st));
		MF_HIP(hipMemsetAsync(p->csc_ptr, 0, ((size_t) p->items + 1) * sizeof(int), st));
		MF_HIP(hipStreamSynchronize(st));
		return MF_OK;
	}
	DevTmp tmp;
	int *d_row = nullptr, *d_col = nullptr, *d_flags = nullptr, *file2csr = nullptr;
	unsigned *key_in = nullptr, *key_out = nullptr, *perm_in = nullptr, *perm_out = nullptr;
	int rc;
	if ((rc = tmp.get(&d_row, nz)) != MF_OK || (rc = tmp.get(&d_col, nz)) != MF_OK ||
	    (rc = tmp.get(&key_in, nz)) != MF_OK || (rc = tmp.get(&key_out, nz)) != MF_OK ||
	    (rc = tmp.get(&perm_in, nz)) != MF_OK || (rc = tmp.get(&perm_out, nz)) != MF_OK ||
	    (rc = tmp.get(&d_flags, 3)) != MF_OK)
		return rc;
	// the values land directly in csr_val when the input is row-sorted (the usual case); otherwise csc_val is
	// used as the staging copy of the file-order values and overwritten last
	double *d_val = p->csc_val;
	double *d_wgt = p->csc_wgt;   // the weights take the same way: csr_wgt first, csc_wgt as the staging copy
	const unsigned grid = (unsigned) ((nnz + 255) / 256);
	if (aos) {
		// one upload of the 16-byte structs, split on the device (no host pass over the entries)
		mf_entry *d_aos = nullptr;
		if ((rc = tmp.get(&d_aos, nz)) != MF_OK) return rc;
		MF_HIP(hipMemcpyAsync(d_aos, aos, nz * sizeof(mf_entry), hipMemcpyHostToDevice, st));
		hipLaunchKernelGGL(split_entries_kernel, dim3(grid), dim3(256), 0, st, d_aos, nnz, swap ? d_col : d_row,
		                   swap ? d_row : d_col, p->csr_val);
	} else {
		MF_HIP(hipMemcpyAsync(d_row, s->row, nz * sizeof(int), hipMemcpyHostToDevice, st));
		MF_HIP(hipMemcpyAsync(d_col, s->col, nz * sizeof(int), hipMemcpyHostToDevice, st));
		MF_HIP(hipMemcpyAsync(p->csr_val, s->val, nz * sizeof(double), hipMemcpyHostToDevice, st));
	}
	if (weight) MF_HIP(hipMemcpyAsync(p->csr_wgt, weight, nz * sizeof(double), hipMemcpyHostToDevice, st));
	MF_HIP(hipMemsetAsync(d_flags, 0, 3 * sizeof(int), st));
	hipLaunchKernelGGL(prep_keys_kernel, dim3(grid), dim3(256), 0, st, d_row, d_col, nnz, p->u0, p->uc, p->items,
	                   key_in, perm_in, d_flags);
	int flags[3] = {0, 0, 0};
	MF_HIP(hipMemcpyAsync(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost, st));
	MF_HIP(hipStreamSynchronize(st));
	if (flags[0]) return MF_ERR_ARGUMENT;
	const bool row_sorted = flags[1] == 0;

	size_t temp_bytes = 0, need = 0;
	MF_HIP(rocprim::radix_sort_pairs(nullptr, need, key_in, key_out, perm_in, perm_out, nz, 0, bits_for(p->uc), st));
	temp_bytes = need;
	MF_HIP(rocprim::radix_sort_pairs(nullptr, need, key_in, key_out, perm_in, perm_out, nz, 0, bits_for(p->items), st));
	temp_bytes = std::max(temp_bytes, need);
	void *d_temp = nullptr;
	if ((rc = tmp.get((char **) &d_temp, temp_bytes)) != MF_OK) return rc;

	const double *vals_file_order = p->csr_val;   // file-order values currently live here
	const double *wgts_file_order = weight ? p->csr_wgt.get() : nullptr;
	if (row_sorted) {
		// CSR == file order: idx = col, val = val (already in place), ptr from the row keys
		MF_HIP(hipMemcpyAsync(p->csr_idx, d_col, nz * sizeof(int), hipMemcpyDeviceToDevice, st));
		hipLaunchKernelGGL(ptr_kernel, dim3((unsigned) ((p->uc + 256) / 256)), dim3(256), 0, st, key_in, nnz, p->uc,
		                   p->csr_ptr);
	} else {
		// keep a file-order copy of the values, then permute into csr_val
		MF_HIP(hipMemcpyAsync(d_val, p->csr_val, nz * sizeof(double), hipMemcpyDeviceToDevice, st));
		vals_file_order = d_val;
		if (weight) {
			MF_HIP(hipMemcpyAsync(d_wgt, p->csr_wgt, nz * sizeof(double), hipMemcpyDeviceToDevice, st));
			wgts_file_order = d_wgt;
		}
		MF_HIP(rocprim::radix_sort_pairs(d_temp, temp_bytes, key_in, key_out, perm_in, perm_out, nz, 0,
		                                 bits_for(p->uc), st));
		hipLaunchKernelGGL(gather_kernel, dim3(grid), dim3(256), 0, st, perm_out, nnz, d_col, 0, vals_file_order,
		                   p->csr_idx, p->csr_val, wgts_file_order, p->csr_wgt.get());
		hipLaunchKernelGGL(ptr_kernel, dim3((unsigned) ((p->uc + 256) / 256)), dim3(256), 0, st, key_out, nnz, p->uc,
		                   p->csr_ptr);
		if (p->want_map) {
			if ((rc = tmp.get(&file2csr, nz)) != MF_OK) return rc;
			hipLaunchKernelGGL(invert_perm_kernel, dim3(grid), dim3(256), 0, st, perm_out, nnz, file2csr);
		}
	}
	// CSC: stable sort of the file order by column
	hipLaunchKernelGGL(copy_keys_kernel, dim3(grid), dim3(256), 0, st, d_col, nnz, key_in, perm_in);
	MF_HIP(rocprim::radix_sort_pairs(d_temp, temp_bytes, key_in, key_out, perm_in, perm_out, nz, 0,
	                                 bits_for(p->items), st));
	if (row_sorted) {
		hipLaunchKernelGGL(gather_kernel, dim3(grid), dim3(256), 0, st, perm_out, nnz, d_row, p->u0, vals_file_order,
		                   p->csc_idx, p->csc_val, wgts_file_order, p->csc_wgt.get());
	} else {
		// vals_file_order aliases csc_val (and the weights' csc_wgt): gather into a temporary, then copy
		double *d_val2 = nullptr, *d_wgt2 = nullptr;
		if ((rc = tmp.get(&d_val2, nz)) != MF_OK) return rc;
		if (weight && (rc = tmp.get(&d_wgt2, nz)) != MF_OK) return rc;
		hipLaunchKernelGGL(gather_kernel, dim3(grid), dim3(256), 0, st, perm_out, nnz, d_row, p->u0, vals_file_order,
		                   p->csc_idx, d_val2, wgts_file_order, d_wgt2);
		MF_HIP(hipMemcpyAsync(p->csc_val, d_val2, nz * sizeof(double), hipMemcpyDeviceToDevice, st));
		if (weight) MF_HIP(hipMemcpyAsync(p->csc_wgt, d_wgt2, nz * sizeof(double), hipMemcpyDeviceToDevice, st));
	}
	hipLaunchKernelGGL(ptr_kernel, dim3((unsigned) ((p->items + 256) / 256)), dim3(256), 0, st, key_out, nnz, p->items,
	                   p->csc_ptr);
	if (!row_sorted || flags[2]) {
		// The recommendation masks rated items by walking a user's item ids in ascending order (print_output's cursor,
		// matFact.c:13-23, relies on (row, col)-sorted input).  The file is not: give the mask its own copy of the ids,
		// ascending inside every row -- the column-sorted sequence, stably re-sorted by row.  The sweeps keep file order.
		unsigned *mk_in = nullptr, *mk_out = nullptr, *mv_out = nullptr;
		if ((rc = tmp.get(&mk_in, nz)) != MF_OK || (rc = tmp.get(&mk_out, nz)) != MF_OK || (rc = tmp.get(&mv_out, nz)) != MF_OK)
			return rc;
		MF_TRY(p->mask_idx.alloc(nz + 64));
		hipLaunchKernelGGL(copy_keys_kernel, dim3(grid), dim3(256), 0, st, p->csc_idx, nnz, mk_in, perm_in);
		size_t need2 = 0;
		MF_HIP(rocprim::radix_sort_pairs(nullptr, need2, mk_in, mk_out, key_out, mv_out, nz, 0, bits_for(p->uc), st));
		void *d_temp2 = d_temp;
		if (need2 > temp_bytes && (rc = tmp.get((char **) &d_temp2, need2)) != MF_OK) return rc;
		MF_HIP(rocprim::radix_sort_pairs(d_temp2, need2, mk_in, mk_out, key_out, mv_out, nz, 0, bits_for(p->uc), st));
		MF_HIP(hipMemcpyAsync(p->mask_idx, mv_out, nz * sizeof(int), hipMemcpyDeviceToDevice, st));
	}
	if (p->want_map) {
		MF_TRY(p->csr2csc.alloc(nz + 64));
		hipLaunchKernelGGL(csr2csc_kernel, dim3(grid), dim3(256), 0, st, perm_out, nnz, file2csr, p->csr2csc);
	}
	MF_HIP(hipGetLastError());
	MF_HIP(hipMemcpyAsync(csr_ptr_host.data(), p->csr_ptr, ((size_t) p->uc + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
	MF_HIP(hipMemcpyAsync(csc_ptr_host.data(), p->csc_ptr, ((size_t) p->items + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
	MF_HIP(hipStreamSynchronize(st));
	return MF_OK;
}


// CSR over the shard's users and CSC over the items, on the device (default) or bucketed on the host
// (MF_BUILD=host, kept for A/B tests); rptr / cptr return the two row-pointer arrays for the schedule decisions.
int build_sparse(mf_plan *p, const mf_shard *s_in, const mf_entry *aos, bool swap, const double *weight, std::vector<int> &rptr,
                 std::vector<int> &cptr)
{
	if (p->cfg.build_host) {   // MF_BUILD=host
		// host fallback of the BUILD only (tests): works on the three arrays
		mf_shard sh = *s_in;
		std::vector<int32_t> hrow, hcol;
		std::vector<double> hval;
		if (aos) {
			try {
				hrow.resize((size_t) sh.nnz);
				hcol.resize((size_t) sh.nnz);
				hval.resize((size_t) sh.nnz);
			} catch (const std::bad_alloc &) {
				return MF_ERR_NO_MEMORY;
			}
			for (int64_t n = 0; n < sh.nnz; ++n) {
				hrow[(size_t) n] = swap ? aos[n].col : aos[n].row;
				hcol[(size_t) n] = swap ? aos[n].row : aos[n].col;
				hval[(size_t) n] = aos[n].value;
			}
			sh.row = hrow.data();
			sh.col = hcol.data();
			sh.val = hval.data();
		}
		const mf_shard *s = &sh;
		for (int64_t n = 0; n < s->nnz; ++n)
			if (s->row[n] < s->user_begin || s->row[n] >= s->user_begin + s->user_count || s->col[n] < 0 ||
			    s->col[n] >= s->items)
				return MF_ERR_ARGUMENT;
		std::vector<int> idx, pos_r, pos_c;
		std::vector<double> val, wgt;
		const size_t nz = (size_t) s->nnz;
		try {
			bucket(s->nnz, p->uc, s->row, p->u0, s->col, 0, s->val, rptr, idx, val, p->want_map ? &pos_r : nullptr, weight, &wgt);
		} catch (const std::bad_alloc &) {
			return MF_ERR_NO_MEMORY;
		}
		MF_TRY(p->csr_ptr.alloc((size_t) p->uc + 1));
		MF_TRY(p->csr_idx.alloc(nz + 64));
		MF_TRY(p->csr_val.alloc(nz + 64));
		MF_HIP(h2d(p, p->csr_ptr, rptr.data(), ((size_t) p->uc + 1) * sizeof(int)));
		{
			// mask ids ascending inside every row (see build_on_device) when the file order is not
			bool ascending = true;
			for (int u = 0; u < p->uc && ascending; ++u)
				ascending = std::is_sorted(idx.begin() + rptr[(size_t) u], idx.begin() + rptr[(size_t) u + 1]);
			if (!ascending) {
				std::vector<int> mk(idx);
				for (int u = 0; u < p->uc; ++u) std::sort(mk.begin() + rptr[(size_t) u], mk.begin() + rptr[(size_t) u + 1]);
				MF_TRY(p->mask_idx.alloc(nz + 64));
				MF_HIP(h2d(p, p->mask_idx, mk.data(), nz * sizeof(int)));
			}
		}
		if (nz) {
			MF_HIP(h2d(p, p->csr_idx, idx.data(), nz * sizeof(int)));
			MF_HIP(h2d(p, p->csr_val, val.data(), nz * sizeof(double)));
		}
		if (weight) {
			MF_TRY(p->csr_wgt.alloc(nz + 64));
			if (nz) MF_HIP(h2d(p, p->csr_wgt, wgt.data(), nz * sizeof(double)));
		}
		try {
			bucket(s->nnz, p->items, s->col, 0, s->row, p->u0, s->val, cptr, idx, val, p->want_map ? &pos_c : nullptr, weight, &wgt);
		} catch (const std::bad_alloc &) {
			return MF_ERR_NO_MEMORY;
		}
		MF_TRY(p->csc_ptr.alloc((size_t) p->items + 1));
		MF_TRY(p->csc_idx.alloc(nz + 64));
		MF_TRY(p->csc_val.alloc(nz + 64));
		MF_HIP(h2d(p, p->csc_ptr, cptr.data(), ((size_t) p->items + 1) * sizeof(int)));
		if (nz) {
			MF_HIP(h2d(p, p->csc_idx, idx.data(), nz * sizeof(int)));
			MF_HIP(h2d(p, p->csc_val, val.data(), nz * sizeof(double)));
		}
		if (weight) {
			MF_TRY(p->csc_wgt.alloc(nz + 64));
			if (nz) MF_HIP(h2d(p, p->csc_wgt, wgt.data(), nz * sizeof(double)));
		}
		if (p->want_map) {
			std::vector<int> map(nz + 1);
			for (size_t n = 0; n < nz; ++n) map[(size_t) pos_r[n]] = pos_c[n];
			MF_TRY(p->csr2csc.alloc(nz + 64));
			if (nz) MF_HIP(h2d(p, p->csr2csc, map.data(), nz * sizeof(int)));
		}
	} else {
		MF_TRY(build_on_device(p, s_in, aos, swap, weight, rptr, cptr));
	}
	return MF_OK;
}

// The inputs of the schedule rules (mf_schedule.h): what the chosen variant can do, the kernel constants, the switches.
mf_sched::Caps schedule_caps(const mf_plan *p)
{
	mf_sched::Caps c;
	c.prod = p->sweep.prod[0] != nullptr, c.pf = p->sweep.has(kPipelined), c.pair = p->sweep.has(kPair), c.coop = p->sweep.has(kCoop), c.db = p->sweep.has(kDb);
	c.row_bytes = p->sweep.row_bytes, c.xs_bytes = p->sweep.xs_bytes, c.single_nch = p->single.nch;
	c.coop_producers = mf::kCoopProducers, c.coop_waves = mf::kCoopWaves, c.slice_cols = mf::kSliceCols;
	c.block_entries = mf::kBlockEntries, c.wave = mf::kWave, c.lds_per_cu = kLdsPerCu;
	return c;
}
mf_sched::Switches schedule_switches(const mf_config &cfg)
{
	mf_sched::Switches w;
	w.skew = cfg.skew, w.sweep_nch = cfg.sweep_nch, w.sweep_long_set = cfg.sweep_long_set, w.sweep_long = cfg.sweep_long;
	w.sweep_pair = cfg.sweep_pair, w.sweep_db = cfg.sweep_db;
	return w;
}

// device copy of a host table (h2d: on the plan's stream, complete on return)
template <class T>
int upload(mf_plan *p, dev_buf<T> &dst, const std::vector<T> &src)
{
	MF_TRY(dst.alloc(src.size()));
	MF_HIP(h2d(p, dst, src.data(), src.size() * sizeof(T)));
	return MF_OK;
}

// Schedule of the two sweeps from the row lengths, by the rules of mf_schedule.h: which rows
// count as long, whether a tiny sweep runs as ONE cooperative launch, the segment tables + scratch buffer of the
// extreme-row path, the wave priority, the form of the main launch and the dispatch order.
int plan_row_schedule(mf_plan *p, const std::vector<int> &rptr, const std::vector<int> &cptr)
{
	// ---- the inputs
	const mf_sched::Caps caps = schedule_caps(p);
	const mf_sched::Switches sw = schedule_switches(p->cfg);
	const mf_sched::Rows rows[2] = {{cptr.data(), p->items}, {rptr.data(), p->uc}};
	mf_sched::Problem pb;
	pb.K = p->K;
	pb.nnz = p->nnz;
	pb.free_bytes = [] {
		size_t free_b = 0, total_b = 0;
		(void) hipMemGetInfo(&free_b, &total_b);
		return free_b;
	};
	// ---- the decision
	const mf_sched::Sweeps s = mf_sched::sweep_schedule(pb, caps, sw, rows);
	// ---- its tables on the device
	for (int kind = 0; kind < 2; ++kind) {
		const mf_sched::Side &h = s.side[kind];
		SweepSide &d = p->side[kind];
		d.max_row_len = h.max_row_len, d.prio_len = h.prio_len, d.long_len = h.long_len;
		d.coop_all = h.coop_all, d.lpt = h.lpt, d.use_db = h.use_db, d.use_pair = h.use_pair;
		if (h.lpt) MF_TRY(upload(p, d.short_rows, h.short_rows));
		if (h.long_rows.empty()) continue;
		d.n_long = (int) h.long_rows.size(), d.n_short = (int) h.short_rows.size(), d.n_seg = (int) h.seg_row.size();
		MF_TRY(upload(p, d.long_rows, h.long_rows));
		MF_TRY(upload(p, d.short_rows, h.short_rows));
		MF_TRY(upload(p, d.seg_row, h.seg_row));
		MF_TRY(upload(p, d.seg_beg, h.seg_beg));
		MF_TRY(upload(p, d.seg_end, h.seg_end));
		MF_TRY(upload(p, d.seg_out, h.seg_out));
		MF_TRY(upload(p, d.lr_sbeg, h.lr_sbeg));
		MF_TRY(upload(p, d.lr_cnt, h.lr_cnt));
	}
	// ---- LDS limits, the scratch, the side stream and its events
	if (s.coop.nch) {
		p->coop = LaunchGeometry{s.coop.nch, s.coop.lds, mf::kCoopWaves * mf::kWave};
		MF_TRY(raise_form_limits(p, kCoop, p->coop.lds));
	}
	if (s.extreme) {
		p->prod = SweepForm{{s.prod_nch, s.prod_lds, mf::kWave}, p->sweep.prod[p->weighted]};
		p->lds_bytes_osum = mf::kOrderedSumLds;
		MF_HIP(raise_lds_limit((const void *) p->prod.fn, p->prod.lds));
		MF_HIP(raise_lds_limit(ordered_sum_fn(p->cfg), p->lds_bytes_osum));
		p->scratch_entries = s.scratch_entries;
		MF_TRY(p->scratch.alloc(p->scratch_entries * mf::kSliceCols * mf_sched::slice_count(p->K, mf::kSliceCols)));
		int prio_lo = 0, prio_hi = 0;
		MF_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
		MF_HIP(hipStreamCreateWithPriority(&p->side_stream, hipStreamNonBlocking, s.side_low ? prio_lo : prio_hi));
		MF_HIP(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
		MF_HIP(hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming));
	}
	return MF_OK;
}

// Item bands of the user sweep: the count by the rule of mf_schedule.h (band_count), and its offset table cut on the device
// from the CSR.  After plan_row_schedule (the form of the side's main launch is an input) and the factor buffers (R's pitch).
int plan_band_tables(mf_plan *p)
{
	SweepSide &us = p->side[1];
	mf_sched::BandInput in;
	in.user_side = true;
	in.sorted = !p->mask_idx;
	in.weighted = p->weighted;
	in.extreme = us.n_long > 0;
	in.single_wave = !us.coop_all && !us.use_db && !us.use_pair;
	in.fixed_k = p->sweep.dma && band_resume_fn(p) != nullptr;
	in.nrows = us.nrows, in.items = p->items;
	in.nnz = p->nnz;
	in.longest_column = p->side[0].max_row_len;
	in.y_bytes = (size_t) p->items * (size_t) p->ldr * sizeof(double);
	in.l2_bytes = kChipL2Bytes;
	in.forced = p->cfg.sweep_bands;
	us.bands = mf_sched::band_count(in);
	if (us.bands < 1) return MF_OK;
	MF_TRY(us.band_off.alloc((size_t) (us.bands + 1) * (size_t) us.nrows));
	hipLaunchKernelGGL(band_offsets_kernel, dim3((unsigned) ((us.nrows + 255) / 256), (unsigned) (us.bands + 1)), dim3(256), 0, p->stream,
	                   p->csr_ptr.get(), p->csr_idx.get(), us.nrows, p->items, us.bands, us.band_off.get());
	MF_HIP(hipGetLastError());
	MF_HIP(raise_lds_limit((const void *) band_resume_fn(p), std::max(p->single.lds, p->few.lds)));
	return MF_OK;
}

// Tables of the errors + streams iteration (mf_stream.hip.h), cut by mf_schedule.h: the CSR rows in segments of at most
// es_nch entries (one wave each in the errors launch) and the workgroup table of the streams launch (mf_resident.hip.h).
int plan_es_schedule(mf_plan *p, const std::vector<int> &rptr, const std::vector<int> &cptr)
{
	p->es_mode = false;
	if (!p->want_map || !p->csr2csc) return MF_OK;
	const mf_sched::Rows rows[2] = {{cptr.data(), p->items}, {rptr.data(), p->uc}};
	const mf_sched::EsErrors e = mf_sched::es_errors(schedule_caps(p), rows[1]);
	if (e.nch < 1) return MF_OK;
	p->es_nch = e.nch;
	p->es_lds_errors = e.lds;
	p->es_nseg = (int) e.seg_row.size();
	if (p->es_nseg == 0 || p->res_sw <= 0) return MF_OK;
	MF_TRY(upload(p, p->es_seg_row, e.seg_row));
	MF_TRY(upload(p, p->es_seg_beg, e.seg_beg));
	MF_TRY(upload(p, p->es_seg_end, e.seg_end));
	MF_TRY(p->rec_csr.alloc((size_t) p->nnz + 64));
	MF_TRY(p->rec_csc.alloc((size_t) p->nnz + 64));
	// records = {idx (fixed), pad, err (rewritten every iteration)}; the 64 entries of slack behind the last one are
	// read (never used) by the streams launch's 64-wide chunk loads
	// on the plan's own stream: it is a non-blocking stream, NOT ordered with the null stream a plain hipMemset runs on
	MF_HIP(hipMemsetAsync(p->rec_csr, 0, ((size_t) p->nnz + 64) * sizeof(mf::StreamRec), p->stream));
	MF_HIP(hipMemsetAsync(p->rec_csc, 0, ((size_t) p->nnz + 64) * sizeof(mf::StreamRec), p->stream));
	{
		const unsigned grid = (unsigned) ((p->nnz + 255) / 256);
		hipLaunchKernelGGL(fill_records_kernel, dim3(grid), dim3(256), 0, p->stream, p->csr_idx, p->nnz, p->rec_csr);
		hipLaunchKernelGGL(fill_records_kernel, dim3(grid), dim3(256), 0, p->stream, p->csc_idx, p->nnz, p->rec_csc);
		MF_HIP(hipGetLastError());
		MF_HIP(hipStreamSynchronize(p->stream));
	}
	MF_HIP(raise_lds_limit((const void *) p->sweep.errs[p->weighted], p->es_lds_errors));
	// ---- LDS-resident streams (mf_resident.hip.h): ~one workgroup per CU
	int ncu = 256;
	{
		hipDeviceProp_t prop;
		if (hipGetDeviceProperties(&prop, p->device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
	}
	const std::vector<mf::SliceWg> wgs =
	    mf_sched::es_workgroups<mf::SliceWg, mf::kResidentWaves>(rows, p->K, p->res_sw, ncu, mf::kResidentRows);
	p->res_nwg = (int) wgs.size();
	p->res_lds = mf_sched::es_resident_lds(std::max(p->uc, p->items), p->res_sw, mf::kResidentWaves, mf::kResidentWaveLds);
	if (p->res_nwg > 0) {
		MF_TRY(upload(p, p->res_wg, wgs));
		MF_HIP(raise_lds_limit(stream_resident_fn(p->res_sw), p->res_lds));
		MF_HIP(raise_lds_limit(stream_resident_fn(p->res_sw, true), p->res_lds));
	}
	p->es_mode = true;
	return MF_OK;
}

}  // namespace
