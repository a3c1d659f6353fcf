"""Device JPEG front-end: the host only reads file bytes; header parsing, Huffman decoding and
the inverse DCT run in libdf3d_hip.so (csrc/jpeg.hip, C ABI `df3d_jpeg_decode_luma`).

Replaces the libjpeg decode inside df2d's DataLoader workers (call site reference df3d/core.py:177-185).  The
result is the JPEG's luma plane with libjpeg's default "islow" IDCT, bit-identical to Pillow / libjpeg-turbo for
grayscale and chroma-neutral files (the rig's monochrome cameras) and to libjpeg's own grayscale output
(`Image.draft("L", ...)`) for coloured ones.

The second half of the file is the encoder: RGB frames on the device -> baseline JPEG files, byte-equal to
Pillow's (csrc/jpeg_encode.hip, C ABI `df3d_jpeg_encode_rgb`); the Motion-JPEG videos are written with it.
"""
import numpy as np
import torch

from . import _native

STATUS = {0: "ok", 1: "truncated file", 2: "not a JPEG", 3: "unsupported JPEG (progressive / arithmetic / 12 bit / multi-scan)",
          4: "corrupt JPEG", 5: "image size differs from the expected one"}


class JpegDecodeError(ValueError):
    pass


def pack_files(blobs, pinned=True):
    """[bytes, ...] -> (uint8 tensor holding the files back to back, each starting on a 16-byte boundary, with 16
    spare bytes at the end; uint32 start offsets [n]; uint32 sizes [n]; total bytes)."""
    sizes = np.array([len(b) for b in blobs], dtype=np.int64)
    ends = np.cumsum((sizes + 15) // 16 * 16)
    starts = ends - (sizes + 15) // 16 * 16
    total = int(ends[-1]) if len(blobs) else 0
    if total >= 2**32 - 64:
        raise ValueError("more than 4 GiB of JPEG data in one batch")
    buf = torch.zeros(total + 16, dtype=torch.uint8)
    if pinned and torch.cuda.is_available():
        buf = buf.pin_memory()
    view = buf.numpy()
    for b, s in zip(blobs, starts):
        view[s : s + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return buf, starts.astype(np.uint32), sizes.astype(np.uint32), total


def decode_luma(blobs, width, height, device=None, check=True, return_status=False, sequential=False, return_path=False):
    """[bytes, ...] of width x height baseline JPEGs -> uint8 CUDA tensor [n, height, width] (luma planes)."""
    _native.require_gpu()
    lib = _native.load()
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    n = len(blobs)
    out = torch.empty((n, height, width), dtype=torch.uint8, device=dev)
    if n == 0:
        extra = ((np.zeros(0, np.int32),) if return_status else ()) + ((np.zeros(0, np.int32),) if return_path else ())
        return (out, *extra) if extra else out
    buf, starts, sizes, total = pack_files(blobs)
    files_dev = buf.to(dev, non_blocking=True)
    tab = torch.from_numpy(np.stack([starts, sizes]).view(np.int32)).to(dev, non_blocking=True)  # [2, n] uint32 bits
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    path = torch.zeros((n,), dtype=torch.int32, device=dev) if return_path else None
    need = lib.df3d_jpeg_work_bytes(n, width, height, total)
    work = torch.empty((need,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):  # kernels launch on the current HIP device
        stream = torch.cuda.current_stream(dev).cuda_stream
        _native.check(
            lib.df3d_jpeg_decode_luma(files_dev.data_ptr(), tab[0].data_ptr(), tab[1].data_ptr(), n, total, int(sizes.max()), width, height, out.data_ptr(),
                                      status.data_ptr(), path.data_ptr() if return_path else None, work.data_ptr(), need, 1 if sequential else 0, stream),
            "df3d_jpeg_decode_luma",
        )
    if check or return_status:
        st = status.cpu().numpy()
        if check and st.any():
            bad = int(np.flatnonzero(st)[0])
            raise JpegDecodeError(f"file {bad} of the batch: {STATUS.get(int(st[bad]), st[bad])}")
        if return_status:
            return (out, st, path.cpu().numpy()) if return_path else (out, st)
    return (out, path.cpu().numpy()) if return_path else out


# pinned staging buffers outlive a reader: page-locking ~80 MB takes longer than decoding a whole batch, and df3d-cli
# (-r / -f) runs one reader per folder.  The pool is bounded by bytes: when a returned buffer does not fit, the smallest
# ones (the least likely to satisfy a later folder's size guess) are dropped first.
_PINNED_POOL = []
PINNED_POOL_MAX_BYTES = 384 << 20


def _pool_put(buf):
    _PINNED_POOL.append(buf)
    _PINNED_POOL.sort(key=lambda b: b.numel())
    while _PINNED_POOL and sum(b.numel() for b in _PINNED_POOL) > PINNED_POOL_MAX_BYTES:
        _PINNED_POOL.pop(0)


def clear_pinned_pool():
    """Release the page-locked staging buffers kept for the next reader (long-lived library users)."""
    del _PINNED_POOL[:]


class JpegFolderReader:
    """Streams JPEG files into the device decoder: the library's native reader threads (df3d_read_files, one call per
    batch, issued from a pool thread) put the files of batch k+1 straight into pinned staging memory while the GPU
    decodes batch k.  Every batch's decode statuses follow it to the host as one asynchronous copy of n int32 on the
    decode's stream; they are looked at when the NEXT batches are submitted (by then the copy has long finished: no
    stall), so a corrupt or unsupported file raises `JpegDecodeError` naming the file within two batches -- not after
    the whole folder has been inferred.  `finish()` checks what is still pending.

        reader = JpegFolderReader(width, height, device)
        for luma in reader.stream(list_of_path_batches):        # uint8 [n, H, W] on the device, decoded on a second stream
            ...                                                 # one batch ahead of the caller's work
        reader.finish()
    (`prefetch` / `decode_next` are the same steps one at a time, on the caller's stream.)
    """

    SLOTS = 3

    def __init__(self, width, height, device=None, workers=None, pinned=True, batch_capacity=None):
        import os
        from concurrent.futures import ThreadPoolExecutor

        _native.require_gpu()
        self.lib = _native.load()
        self.dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.width, self.height = int(width), int(height)
        self.pinned = bool(pinned)
        self.pool = ThreadPoolExecutor(max_workers=workers or self.SLOTS)  # one task per batch being read; the reading itself is native
        self.slots = [dict(buf=None, event=None) for _ in range(self.SLOTS)]
        self.turn = 0
        self.queue = []     # batches being read, oldest first (at most SLOTS - 1: one staging buffer may still feed a copy)
        self.work = None
        self.batch_capacity = batch_capacity  # largest batch `stream()` will see (None: the first batch is the largest)
        self.side = None    # second HIP stream of `stream()`: H2D copies + decode kernels under the caller's compute
        self._keep = None
        self.pending = []   # (event, pinned host statuses, n, paths) of decoded batches whose statuses have not been looked at
        self._status_host = []  # pinned int32 buffers, recycled

    READ_THREADS = 8  # native reader threads per batch (two batches may be in flight)

    def _pinned(self, nbytes):
        return torch.empty(int(nbytes), dtype=torch.uint8, pin_memory=self.pinned)

    def _read_batch(self, slot, paths):
        """The files of one batch -> the slot's staging buffer through df3d_read_files (native threads open, size and read
        them; run from a pool thread, the interpreter lock is free meanwhile).  Returns (rc, starts, sizes, total bytes);
        rc = DF3D_ENOSPC: nothing was read, the buffer must hold total + 16 bytes (the caller, on the main thread, makes
        one: pinned allocations from a fresh thread cost hundreds of milliseconds)."""
        import ctypes
        import os

        n = len(paths)
        arr = (ctypes.c_char_p * n)(*[os.fsencode(p) for p in paths])
        starts, sizes = np.empty(n, np.uint32), np.empty(n, np.uint32)
        total = ctypes.c_size_t(0)
        buf = slot["buf"]
        rc = self.lib.df3d_read_files(arr, n, buf.data_ptr() if buf is not None else None, buf.numel() if buf is not None else 0, starts.ctypes.data,
                                      sizes.ctypes.data, ctypes.byref(total), self.READ_THREADS)
        if rc == _native.DF3D_EIO:
            msg = self.lib.df3d_last_error().decode()
            raise (FileNotFoundError if "No such file" in msg else IOError)(msg)
        if rc != _native.DF3D_ENOSPC:
            _native.check(rc, "df3d_read_files")
        return rc, starts, sizes, int(total.value)

    def prefetch(self, paths, sizes=None):
        """Start reading `paths` into the next staging slot (`sizes` is accepted for callers of round 1 and ignored: the native
        reader sizes the files as it opens them)."""
        import os

        if len(self.queue) >= self.SLOTS - 1:
            raise RuntimeError("too many batches are being read")
        slot = self.slots[self.turn]
        self.turn = (self.turn + 1) % self.SLOTS
        if slot["event"] is not None:
            slot["event"].synchronize()  # the copy that last used this staging buffer has finished
        paths = list(paths)
        if paths:
            # room for the batch if its files are like the first one (camera frames are); a wrong guess costs one re-read
            guess = int(max(len(paths), self.batch_capacity or 0) * (os.stat(paths[0]).st_size + 16) * 1.25) + 4096
            if slot["buf"] is None and self.pinned:
                fit = [b for b in _PINNED_POOL if b.numel() >= guess]
                if fit:
                    slot["buf"] = min(fit, key=lambda b: b.numel())
                    _PINNED_POOL[:] = [b for b in _PINNED_POOL if b is not slot["buf"]]
            if slot["buf"] is None or slot["buf"].numel() < guess:
                slot["buf"] = self._pinned(guess)
        self.queue.append((slot, self.pool.submit(self._read_batch, slot, paths) if paths else None, paths))

    def _launch_decode(self, out, stream):
        """Wait for the batch being read and enqueue its H2D copy + decode on `stream` into `out[:n]`."""
        self.check_statuses()   # of the batches decoded before: fail within two batches of a bad file
        slot, fut, paths = self.queue.pop(0)
        n = len(paths)
        if n:
            rc, starts, sizes, total = fut.result()
            if rc == _native.DF3D_ENOSPC:  # the size guess was too small
                slot["buf"] = self._pinned((total + 16) * 1.25)
                rc, starts, sizes, total = self._read_batch(slot, paths)
                _native.check(rc, "df3d_read_files")
            if total >= 2**32 - 64:
                raise ValueError("more than 4 GiB of JPEG data in one batch")
        if n:
            with torch.cuda.device(self.dev), torch.cuda.stream(stream):
                files_dev = slot["buf"][: total + 16].to(self.dev, non_blocking=True)
                tab = torch.from_numpy(np.stack([starts, sizes]).view(np.int32)).to(self.dev, non_blocking=True)
                slot["event"] = torch.cuda.Event()
                slot["event"].record(stream)
                status = torch.empty((n,), dtype=torch.int32, device=self.dev)
                need = self.lib.df3d_jpeg_work_bytes(n, self.width, self.height, total)
                if self.work is None or self.work.numel() < need:
                    self.work = torch.empty((need,), dtype=torch.uint8, device=self.dev)
                _native.check(
                    self.lib.df3d_jpeg_decode_luma(files_dev.data_ptr(), tab[0].data_ptr(), tab[1].data_ptr(), n, total, int(sizes.max()), self.width,
                                                   self.height, out.data_ptr(), status.data_ptr(), None, self.work.data_ptr(), self.work.numel(), 0,
                                                   stream.cuda_stream),
                    "df3d_jpeg_decode_luma",
                )
                self._keep = (files_dev, tab, status)  # alive until the next launch on this stream has been enqueued behind them
                host = self._status_host.pop() if self._status_host else None
                if host is None or host.numel() < n:
                    host = torch.empty(max(n, self.batch_capacity or 0), dtype=torch.int32, pin_memory=self.pinned)
                host[:n].copy_(status, non_blocking=True)
                done = torch.cuda.Event()
                done.record(stream)
            self.pending.append((done, host, n, paths))
        return n

    def check_statuses(self, wait=False):
        """Look at the decode statuses that have reached the host: every batch but the newest one is waited for (its decode
        was enqueued at least one batch ago), the newest only if `wait`.  Raises JpegDecodeError naming the first bad file."""
        while self.pending:
            done, host, n, paths = self.pending[0]
            if not (wait or len(self.pending) > 1 or done.query()):
                break
            done.synchronize()
            self.pending.pop(0)
            st = host[:n].numpy()
            bad = np.flatnonzero(st)
            if bad.size:
                b = int(bad[0])
                raise JpegDecodeError(f"{paths[b]}: {STATUS.get(int(st[b]), st[b])}")
            self._status_host.append(host)

    def decode_next(self, next_paths=None):
        """Wait for the batch being read, launch its decode, start reading `next_paths`; returns luma [n, H, W]."""
        n = len(self.queue[0][2])
        out = torch.empty((n, self.height, self.width), dtype=torch.uint8, device=self.dev)
        self._launch_decode(out, torch.cuda.current_stream(self.dev))
        if next_paths is not None:
            self.prefetch(next_paths)
        return out

    def stream(self, batches, sizes=None):
        """Generator over the decoded batches of `batches` (a list of path lists), pipelined three deep: while the caller's
        stream works on batch k (everything it enqueues between two `next()` calls), batch k + 1 is copied and decoded on a
        second HIP stream and the files of batch k + 2 are read by the thread pool.  Each yielded tensor (uint8 [n, H, W],
        one of two alternating device buffers) is valid on the caller's current stream until the next item is requested.  `sizes[k]`: byte sizes of batch k's files."""
        if not len(batches):
            return
        main = torch.cuda.current_stream(self.dev)
        if self.side is None:
            self.side = torch.cuda.Stream(device=self.dev)
        side = self.side
        first = batches[0]
        cap = max(len(first), self.batch_capacity or 0)
        luma = [torch.empty((cap, self.height, self.width), dtype=torch.uint8, device=self.dev) for _ in range(2)]
        for buf in luma:
            buf.record_stream(side)   # written on the side stream: if the consumer abandons the generator the allocator must not
                                      # hand the memory out again before that stream is done with it
        side.wait_stream(main)  # the buffers exist for the side stream
        decoded, consumed = [None, None], [None, None]
        size_of = (lambda k: None) if sizes is None else (lambda k: sizes[k])
        self.prefetch(first, size_of(0))
        if len(batches) > 1:
            self.prefetch(batches[1], size_of(1))   # both reads are under way before the first one is waited for
        n_cur = self._launch_decode(luma[0], side)
        decoded[0] = torch.cuda.Event()
        decoded[0].record(side)
        for k in range(len(batches)):
            main.wait_event(decoded[k & 1])
            yield luma[k & 1][:n_cur]
            consumed[k & 1] = torch.cuda.Event()
            consumed[k & 1].record(main)  # everything the caller enqueued on batch k
            if k + 1 < len(batches):
                nb = (k + 1) & 1
                if k + 2 < len(batches):
                    self.prefetch(batches[k + 2], size_of(k + 2))   # before waiting for batch k + 1's reads
                if consumed[nb] is not None:
                    side.wait_event(consumed[nb])  # batch k - 1 no longer reads this buffer
                n_cur = self._launch_decode(luma[nb], side)
                decoded[nb] = torch.cuda.Event()
                decoded[nb].record(side)
        main.wait_stream(side)

    def finish(self, check=True):
        """Check the decode statuses still pending (one host synchronisation) and release the reader threads.  `check=False`
        on an error path: release only (the exception under way is the one to report)."""
        try:
            if check:
                self.check_statuses(wait=True)
        finally:
            self.pending = []
            self.pool.shutdown(wait=False)
            for item in self.queue:  # an error path: file reads may still be writing into a staging buffer
                try:
                    if item[1] is not None:
                        item[1].result()
                except Exception:
                    pass
            self.queue = []
            if self.pinned:
                for slot in self.slots:
                    if slot["event"] is not None:
                        slot["event"].synchronize()  # the last copy out of this buffer has finished
                    if slot["buf"] is not None:
                        _pool_put(slot["buf"])
                    slot["buf"] = None


# ---- the encoder ------------------------------------------------------------------------------------------------
# libjpeg's baseline encoder on the device (csrc/jpeg_encode.hip, C ABI `df3d_jpeg_encode_rgb`): 4:2:0, the Annex K tables, no restart
# markers.  The device writes the entropy-coded scan; the header and EOI are put around it here.  Byte-equal to Pillow's
# `save(format="JPEG", quality=q)`.
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36,
          29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68,
              109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# the Annex K Huffman tables as DHT segment bodies: class/id, 16 counts, the symbols
_DHT = (
    bytes([0x00, 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]) + bytes(range(12)),
    bytes([0x10, 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]) + bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
        "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
        "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    bytes([0x01, 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]) + bytes(range(12)),
    bytes([0x11, 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]) + bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
        "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4"
        "c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"),
)
assert all(len(t) == 17 + sum(t[1:17]) for t in _DHT)


def _quality(quality):
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError(f"quality must be an integer 1 .. 100, got {quality!r}")
    return q


def quality_tables(quality):
    """libjpeg's quantisation tables for `quality` (1 .. 100): (luma, chroma), each [64] uint8 in natural order."""
    q = _quality(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(base, dtype=np.int64) * scale + 50) // 100, 1, 255).astype(np.uint8) for base in (_BASE_LUMA, _BASE_CHROMA))


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


def jfif_header(width, height, quality):
    """Everything in front of the scan, in the order libjpeg (Pillow) writes it: SOI, APP0 (JFIF 1.1), two DQT, SOF0 (4:2:0), four DHT, SOS."""
    if not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
        raise ValueError(f"width and height must be 1 .. 65535, got {width} x {height}")
    luma, chroma = quality_tables(quality)
    zz = list(ZIGZAG)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += _segment(0xDB, b"\0" + luma[zz].tobytes()) + _segment(0xDB, b"\1" + chroma[zz].tobytes())
    out += _segment(0xC0, bytes([8]) + int(height).to_bytes(2, "big") + int(width).to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for table in _DHT:
        out += _segment(0xC4, table)
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0]))


def blocks_per_frame(width, height):
    """8 x 8 blocks in a frame's scan, the dummy ones that fill the last MCUs included."""
    return 6 * ((width + 15) // 16) * ((height + 15) // 16)


def encode_scans(frames, tables, out, sizes, status, work, coef=None, bits=None):
    """One `df3d_jpeg_encode_rgb` call on the current stream: frames [n, H, W, 3] uint8 cuda, contiguous -> out [n, capacity] uint8 (the scans),
    sizes [n] int64, status [n] int32; `coef` [n, blocks, 64] int16 and `bits` [n, blocks] int32 take the stages when given."""
    lib = _native.load()
    n, h, w, _ = frames.shape
    luma, chroma = (np.ascontiguousarray(t, dtype=np.uint8) for t in tables)
    with torch.cuda.device(frames.device):
        _native.check(
            lib.df3d_jpeg_encode_rgb(frames.data_ptr(), n, h, w, luma.ctypes.data, chroma.ctypes.data, out.data_ptr(), out.shape[1], sizes.data_ptr(),
                                     status.data_ptr(), work.data_ptr(), work.numel(), coef.data_ptr() if coef is not None else None,
                                     bits.data_ptr() if bits is not None else None, torch.cuda.current_stream(frames.device).cuda_stream),
            "df3d_jpeg_encode_rgb",
        )


class JpegFrameEncoder:
    """Encodes batches of up to `batch` RGB frames of one size on the device and returns their JPEG files.  The work area, the output slots
    and a pinned host buffer persist across calls.  Per batch: one launch sequence, then the sizes and the first `fetch` bytes of every slot
    cross to the host behind one synchronisation (`fetch` is 1.25 x the largest scan seen so far; a batch that outgrows it costs one more copy).
    The slots' capacity starts as a guess: a frame that does not fit is encoded again with the size the device reported, never truncated."""

    def __init__(self, width, height, batch=16, quality=90, device=None, capacity=None):
        _native.require_gpu()
        self.lib = _native.load()
        self.dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.dev.type == "cuda" and self.dev.index is None:   # "cuda": the current device, by its index (tensors carry one)
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.w, self.h, self.batch, self.quality = int(width), int(height), int(batch), _quality(quality)
        if self.batch < 1:
            raise ValueError("batch must be at least 1")
        self.tables = quality_tables(self.quality)
        self.header = jfif_header(self.w, self.h, self.quality)
        need = self.lib.df3d_jpeg_encode_work_bytes(self.batch, self.w, self.h)
        if need == 0:
            raise ValueError(f"a {self.w} x {self.h} frame is outside what the encoder takes: {self.lib.df3d_last_error().decode() or 'size'}")
        self.work = torch.empty((need,), dtype=torch.uint8, device=self.dev)
        self.meta = torch.zeros((2 * self.batch,), dtype=torch.int64, device=self.dev)   # sizes, then the statuses (int32) in the second half
        self.meta_host = torch.zeros((2 * self.batch,), dtype=torch.int64).pin_memory()
        self.retries = 0
        self.largest = 0     # the largest scan seen so far
        self._room(capacity if capacity is not None else self.w * self.h // 4 + 4096)

    def _room(self, capacity):
        self.capacity = (int(capacity) + 255) // 256 * 256
        self.out = torch.empty((self.batch, self.capacity), dtype=torch.uint8, device=self.dev)
        self.host = torch.empty((self.batch * self.capacity,), dtype=torch.uint8).pin_memory()

    @property
    def fetch(self):
        """Bytes of every slot that cross to the host with the sizes: the whole slot until a scan has been seen, then 1.25 x the largest."""
        if not self.largest:
            return self.capacity
        return min(self.capacity, max(4096, (self.largest + self.largest // 4 + 255) // 256 * 256))

    def encode(self, frames):
        """frames [n, H, W, 3] uint8 on the encoder's device, n <= batch -> [bytes, ...]: n whole JPEG files."""
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4):
            raise ValueError("frames must be a [n, H, W, 3] uint8 CUDA tensor")
        if frames.device != self.dev or tuple(frames.shape[1:]) != (self.h, self.w, 3) or frames.shape[0] > self.batch:
            raise ValueError(f"frames must be [<= {self.batch}, {self.h}, {self.w}, 3] on {self.dev}, got {list(frames.shape)} on {frames.device}")
        n = frames.shape[0]
        if n == 0:
            return []
        frames = frames.contiguous()
        sizes, status = self.meta[:self.batch], self.meta[self.batch:].view(torch.int32)[:self.batch]
        while True:
            encode_scans(frames, self.tables, self.out, sizes, status, self.work)
            self.meta_host.copy_(self.meta, non_blocking=True)
            fetched = self.fetch
            rows = self.host[:n * fetched].view(n, fetched)
            rows.copy_(self.out[:n, :fetched], non_blocking=True)
            torch.cuda.current_stream(self.dev).synchronize()
            size = self.meta_host[:n].numpy()
            biggest = int(size.max())
            if biggest <= self.capacity:
                break
            self.retries += 1
            self._room(biggest + biggest // 8)     # the reported size, and some room for the frames that follow
        if biggest > fetched:                      # the guess of how much to fetch was too small for this batch
            rows = self.host[:n * biggest].view(n, biggest)
            rows.copy_(self.out[:n, :biggest])
        self.largest = max(self.largest, biggest)
        view = rows.numpy()
        return [self.header + view[i, :int(size[i])].tobytes() + b"\xff\xd9" for i in range(n)]


def encode_rgb(frames, quality=90):
    """[n, H, W, 3] or [H, W, 3] uint8 cuda -> [bytes, ...]: the frames' baseline JPEG files (4:2:0), byte-equal to Pillow's at that quality."""
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() in (3, 4) and frames.shape[-1] == 3):
        raise ValueError("frames must be a [n, H, W, 3] or [H, W, 3] uint8 CUDA tensor")
    if frames.dim() == 3:
        frames = frames[None]
    n, h, w, _ = frames.shape
    if n == 0:
        return []
    return JpegFrameEncoder(w, h, batch=n, quality=quality, device=frames.device).encode(frames)
