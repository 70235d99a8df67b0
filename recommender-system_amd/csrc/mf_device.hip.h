// mf_device.hip.h -- the HIP error macro and device memory: dev_alloc and the owner dev_buf<T>.  Every hipMalloc and
// hipFree of the library is in this file.
#pragma once

namespace {

thread_local std::string g_last_hip_error;

#define MF_HIP(call)                                                                        \
	do {                                                                                    \
		hipError_t _e = (call);                                                             \
		if (_e != hipSuccess) {                                                             \
			g_last_hip_error = std::string(#call) + ": " + hipGetErrorString(_e);           \
			return _e == hipErrorOutOfMemory ? MF_ERR_NO_MEMORY : MF_ERR_HIP;               \
		}                                                                                   \
	} while (0)

// inside functions that return a status: pass a failure on
#define MF_TRY(x)                     \
	do {                              \
		int _rc = (x);                \
		if (_rc != MF_OK) return _rc; \
	} while (0)

template <typename T>
int dev_alloc(T **out, size_t count)
{
	*out = nullptr;
	MF_HIP(hipMalloc((void **) out, std::max<size_t>(count, 1) * sizeof(T)));
	return MF_OK;
}

// Owner of one device allocation: the pointer and its capacity in elements.  Move-only; converts to T* so that it
// reads like the pointer at kernel-argument sites; frees on destruction.  A failed alloc / grow leaves it empty.
template <typename T>
class dev_buf {
	T *ptr_ = nullptr;
	size_t cap_ = 0;

public:
	dev_buf() = default;
	dev_buf(const dev_buf &) = delete;
	dev_buf &operator=(const dev_buf &) = delete;
	dev_buf(dev_buf &&o) noexcept : ptr_(o.ptr_), cap_(o.cap_) { o.ptr_ = nullptr, o.cap_ = 0; }
	dev_buf &operator=(dev_buf &&o) noexcept
	{
		if (this != &o) {
			reset();
			ptr_ = o.ptr_, cap_ = o.cap_;
			o.ptr_ = nullptr, o.cap_ = 0;
		}
		return *this;
	}
	~dev_buf() { reset(); }

	operator T *() const { return ptr_; }
	T *get() const { return ptr_; }
	size_t capacity() const { return cap_; }

	void reset()
	{
		if (ptr_) (void) hipFree(ptr_);
		ptr_ = nullptr;
		cap_ = 0;
	}
	int alloc(size_t count)
	{
		reset();
		const int rc = dev_alloc(&ptr_, count);
		if (rc == MF_OK) cap_ = count;
		return rc;
	}
	// at least `count` elements; the contents are not kept
	int grow(size_t count) { return cap_ >= count ? MF_OK : alloc(count); }
};

// Buffers that share a capacity grow together: a failure leaves all of them empty, so the next call allocates all again.
template <typename... B>
int grow_all(size_t count, B &...bufs)
{
	int rc = MF_OK;
	((rc = rc == MF_OK ? bufs.grow(count) : rc), ...);
	if (rc != MF_OK) (bufs.reset(), ...);
	return rc;
}

}  // namespace
