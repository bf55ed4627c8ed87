"""`TesterUnited` on the MI355X engine: the reference's test harness for channel==4 models
(testing/tester.py:17-108, testing/tester_single.py:34-42, testing/tester_united.py:15-195) with the same directory
layout, container files, bpp / PSNR arithmetic, timing windows and log lines, so `playground/test.py -m ELIC_united
--channel 4 -q 2_2 -d <dataset>` has a drop-in target.  Image I/O uses PIL (cv2 / torchvision are not required).
"""
import io
import logging
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from .arch import mlic_config, model_config
from .datautils import crop0, crop1, pad
from .ioutils import filesize, read_body, read_uints, write_body, write_uints
from .metrics import AverageMeter, compute_metrics, finish_metrics, metrics_batch


def save_image(x, path):
    """utils/IOutils.py:101-104 (ToPILImage of the clamped tensor): uint8 PNG, value*255 truncated like torchvision's
    `pic.mul(255).byte()`."""
    from PIL import Image

    a = x.detach().clamp(0, 1).squeeze(0).mul(255).byte().cpu().numpy()
    Image.fromarray(a[0] if a.shape[0] == 1 else a.transpose(1, 2, 0)).save(path)


def save_depth16(x, path, scale):
    """tester_united.py:101-109: depth * 10000 (NYUv2) or * 100000 (SUN RGB-D) as a 16-bit PNG."""
    from PIL import Image

    Image.fromarray((x.detach() * scale).cpu().squeeze().numpy().astype("uint16")).save(path)


def load_image(path, mode):
    """dataset/testDataset.py:36-61: RGB/255; depth scaled by 10000 / 100000 / 255 depending on its range."""
    from PIL import Image

    img = np.array(Image.open(path))
    if mode == "RGB":
        if img.ndim == 2:
            img = np.stack([img] * 3, -1)
        t = torch.from_numpy(np.ascontiguousarray(img[..., :3].transpose(2, 0, 1))).float() / 255.0
    else:
        t = torch.from_numpy(img.astype("float32"))[None]
        mx = float(t.max())
        t = t / (10000.0 if 255 < mx < 10000 else (100000.0 if mx > 10000 else 255.0))
    return t


class ImageFolderUnited:
    """Pairs <root>/rgb/* with <root>/depth/* by sorted file name (dataset/testDataset.py:14-79)."""

    def __init__(self, root, debug=False):
        self.rgb = sorted(f for f in (Path(root) / "rgb").iterdir() if f.is_file())
        self.depth = sorted(f for f in (Path(root) / "depth").iterdir() if f.is_file())
        if not self.rgb or len(self.rgb) != len(self.depth):
            raise RuntimeError(f'Invalid directory "{root}"')
        if debug:
            self.rgb, self.depth = self.rgb[:20], self.depth[:20]

    def __len__(self):
        return len(self.rgb)

    def __getitem__(self, i):
        return (load_image(self.rgb[i], "RGB")[None], load_image(self.depth[i], "L")[None],
                [os.path.splitext(self.rgb[i].name)[0]], [os.path.splitext(self.depth[i].name)[0]])


class TesterUnited:
    def __init__(self, args, config=None, net=None):
        self.device = "cuda"
        self.channel = args.channel
        self.debug = getattr(args, "debug", False)
        self.exp_name = args.experiment or self.get_exp_name(args.dataset, args.channel, args.model, args.quality)
        self.exp_dir_path = os.path.join("../experiments_test" if self.debug else "../experiments", self.exp_name)
        self.ckpt_dir_path = os.path.join(self.exp_dir_path, "checkpoints")
        # (playground/test.py:29-32: a model name with "MLIC" in it selects MLIC_model_config())
        self.model_config = config or (mlic_config() if str(args.model).find("MLIC") != -1 else model_config())
        self.net = net
        self.epoch = 0
        if net is None:
            self.epoch = self.get_net(self.model_config, args.model, args.checkpoint)
        self.logger_test = logging.getLogger("test")
        self.test_dataloader = ImageFolderUnited(args.dataset, debug=self.debug) if args.dataset else None
        self.save_dir = os.path.join(self.exp_dir_path, "codestream")

    # tester.py:55-108
    def get_net(self, model_config_, model_name, ckpt_path):
        from . import elic_united

        model = elic_united.zoo_lookup(model_name)  # modelZoo, then the younger entries (rgbd_amd.zoo_lookup)
        if model is None:
            raise ValueError(f"model {model_name} is not provided by rgbd_amd (ELIC_united and ELIC only)")
        self.net = model(config=model_config_, channel=self.channel).eval()
        best = os.path.join(self.ckpt_dir_path, "checkpoint_best_loss.pth.tar")
        if ckpt_path is None and os.path.exists(best):
            ckpt_path = best
        checkpoint = torch.load(ckpt_path, map_location="cpu")
        self.net.load_state_dict(checkpoint["state_dict"])
        self.net.update(force=True)
        self.net = self.net.to(self.device)
        return checkpoint["epoch"]

    @staticmethod
    def get_exp_name(dataset, channel, model_name, quality):
        modal = {1: "depth_", 3: "rgb_", 4: ""}[channel]
        return f"{'nyuv2' if dataset.find('nyu') != -1 else 'sunrgbd'}_{modal}{model_name}_{quality}"

    def get_rec_dir(self, padding=True, padding_mode="reflect0"):
        rec_dir = os.path.join(self.save_dir, f"{self.epoch}-padding-{padding_mode}" if padding else f"{self.epoch}-CenterCrop")
        for d in (rec_dir, os.path.join(rec_dir, "depth_rec"), os.path.join(rec_dir, "rgb_rec")):
            os.makedirs(d, exist_ok=True)
        return rec_dir

    # tester_united.py:141-167
    def compress_one_image_united(self, x, stream_path, H, W, img_name, net=None, sync=torch.cuda.synchronize):
        net = net or self.net
        sync()
        start = time.time()
        out = net.compress(x[0], x[1])
        sync()
        enc_time = time.time() - start
        bpps = []
        for path, key in ((stream_path[0], "r_strings"), (stream_path[1], "d_strings")):
            os.makedirs(path, exist_ok=True)
            fn = os.path.join(path, img_name)
            with Path(fn).open("wb") as f:
                write_uints(f, (H, W))
                write_body(f, out["shape"], out[key])
            bpps.append(float(filesize(fn)) * 8 / (H * W))
        return bpps[0], bpps[1], enc_time

    # tester_united.py:169-195
    def decompress_one_image_united(self, stream_path, img_name, mode="reflect0", net=None, sync=torch.cuda.synchronize):
        net = net or self.net
        strings = []
        for path in stream_path:
            with Path(os.path.join(path, img_name)).open("rb") as f:
                original_size = read_uints(f, 2)
                s, shape = read_body(f)
                strings.append(s)
        sync()
        start = time.time()
        out = net.decompress(strings[0], strings[1], shape)
        sync()
        dec_time = time.time() - start
        cropper = crop0 if mode.find("0") != -1 else crop1
        return cropper(out["x_hat"]["r"], original_size), cropper(out["x_hat"]["d"], original_size), dec_time

    # tester_united.py:48-88 (the rgb stream really lands in "depth_bin" and vice versa, :62-63)
    def _one_image(self, i, rec_dir, padding_mode, net=None, sync=torch.cuda.synchronize):
        rgb, depth, rgb_name, _ = self.test_dataloader[i]
        _, _, H, W = rgb.shape
        rgb, depth = rgb.to(self.device), depth.to(self.device)
        paths = (os.path.join(rec_dir, "depth_bin"), os.path.join(rec_dir, "rgb_bin"))
        rb, db, et = self.compress_one_image_united((pad(rgb, padding_mode), pad(depth, padding_mode)), paths, H, W,
                                                    rgb_name[0], net=net, sync=sync)
        xr, xd, dt = self.decompress_one_image_united(paths, rgb_name[0], mode=padding_mode, net=net, sync=sync)
        rp, rm = compute_metrics(xr, rgb)
        dp, dm = compute_metrics(xd, depth)
        if getattr(self, "save_reconstructions", True):  # tester_united.py:98-109
            save_image(xr, os.path.join(rec_dir, "rgb_rec", f"{rgb_name[0]}_{rb:.4f}_{rp:.4f}__rec.png"))
            save_image(xd, os.path.join(rec_dir, "depth_rec", f"{rgb_name[0]}_{db:.4f}_{dp:.4f}__rec_8bit.png"))
            save_depth16(xd, os.path.join(rec_dir, "depth_rec", f"{rgb_name[0]}_{db:.4f}_{dp:.4f}__rec_16bit.png"),
                         100000 if rec_dir.find("sun") != -1 else 10000)
        return rgb_name[0], H * W, (rp, rm, rb, dp, dm, db, dt, et)

    def _test_pipelined(self, results, rec_dir, padding_mode, W, batch=4):
        """W engine instances in flight, each coding up to `batch` consecutive images of one size per call (SURVEY 8f rank 1:
        the steps either side of the codec become the bottleneck once enc + dec is ~100 ms).  Three kinds of threads, so that
        nothing but the engine calls sits on an image's critical path:
          * decoders (PIL inflates PNGs and numpy / torch-CPU normalise with the GIL released) run a bounded distance ahead;
          * W GPU workers, one engine instance + HIP stream each: pad on the GPU, ONE compress() for the group with per-image
            streams (bit-identical to one call per image: the kernels are batch-invariant, tests/test_gpu_parity_pinned.py),
            one container image per picture, ONE decompress() of exactly those bytes (parsed back from the container images
            that go to disk), crop, clamp, PSNR / MS-SSIM on the GPU with one small copy back per picture, uint8 / int
            conversion of the reconstructions on the GPU;
          * writers put the container files and (save_reconstructions) the PNGs on disk.
        Files, bpp and PSNR are those of the one-at-a-time loop (tests/test_gpu_harness.py); the per-image latencies are the
        group's windows divided by its size."""
        from PIL import Image

        n = len(results)
        ds = self.test_dataloader
        # groups of consecutive images with the same size (header reads only)
        sizes = [Image.open(ds.rgb[i]).size for i in range(n)]
        units, cur = [], []
        for i in range(n):
            if cur and (len(cur) >= batch or sizes[i] != sizes[cur[0]]):
                units.append(cur)
                cur = []
            cur.append(i)
        if cur:
            units.append(cur)
        W = max(1, min(W, len(units)))
        # engine instances are kept between calls: a clone's first call of a shape sizes its workspace, the second captures
        # its HIP graphs, only the third replays -- a second test_model() (or a long dataset) runs warm
        pool = getattr(self, "_pool_nets", None)
        if pool is None or pool[0] is not self.net:
            pool = [self.net]
        from .sched import check_hw_queues

        check_hw_queues()  # refuses a queue count above sched.MAX_SAFE_HW_QUEUES: launches on other streams were seen to fail there
        while len(pool) < W:
            pool.append(self.net.clone_shared())
        self._pool_nets = pool
        nets = pool[:W]
        blocking = W > 1 and os.environ.get("RGBD_BLOCKING_SYNC", "1") != "0"  # W host threads wait on W streams: sleep, do not spin
        if blocking:
            from ._lib import set_blocking_sync

            set_blocking_sync(True)
        was_per_image = self.net.per_image_streams
        for nt in nets:
            nt.per_image_streams = True
            if W >= 4:
                nt.set_tile_mode("throughput")
        dev = torch.device("cuda", torch.cuda.current_device())
        save = getattr(self, "save_reconstructions", True)
        scale16 = 100000 if rec_dir.find("sun") != -1 else 10000
        paths = (os.path.join(rec_dir, "depth_bin"), os.path.join(rec_dir, "rgb_bin"))  # (sic: tester_united.py:62-63)
        for p_ in paths:
            os.makedirs(p_, exist_ok=True)
        ahead = threading.Semaphore(3 * W * batch)  # decoded images waiting for a GPU worker
        decoders = ThreadPoolExecutor(max_workers=max(2, min(8, W * batch)))
        writers = ThreadPoolExecutor(max_workers=max(2, min(12, 2 * W)))

        def decode(i):
            ahead.acquire()
            return ds[i]  # load_image(): the floats of the one-at-a-time loop

        order = [i for u in units for i in u]  # decode in the order the workers will ask
        futs = {}
        for w0 in range(0, len(units), W):  # round-robin over the workers: unit k goes to worker k % W
            for u in units[w0:w0 + W]:
                for i in u:
                    futs[i] = decoders.submit(decode, i)
        assert len(futs) == len(order)
        pending, errs = [], [None] * W
        stage = [dict() for _ in range(W)]  # host seconds per pipeline stage and worker (self.stage_seconds: where a job's time goes)

        def tick(w, name, t0):
            t1 = time.time()
            stage[w][name] = stage[w].get(name, 0.0) + (t1 - t0)
            return t1

        def write_file(fn, data):
            with open(fn, "wb") as f:
                f.write(data)

        def write_png(arr, fn, as16=False):
            Image.fromarray(arr.astype("uint16") if as16 else arr).save(fn)

        def work(w):
            try:
                torch.cuda.set_device(dev)
                stream = torch.cuda.Stream(device=dev)
                net = nets[w]
                with torch.cuda.stream(stream), torch.no_grad():
                    for u in units[w::W]:
                        ts = time.time()
                        items = []
                        for i in u:
                            items.append(futs[i].result())
                            ahead.release()
                        ts = tick(w, "wait_decode", ts)
                        k = len(u)
                        rgb = torch.cat([it[0] for it in items]).to(dev)
                        depth = torch.cat([it[1] for it in items]).to(dev)
                        names = [it[2][0] for it in items]
                        H, Wd = rgb.shape[-2:]
                        rp_, dp_ = pad(rgb, padding_mode), pad(depth, padding_mode)
                        stream.synchronize()
                        ts = tick(w, "upload_pad", ts)
                        t0 = time.time()
                        out = net.compress(rp_, dp_)
                        stream.synchronize()
                        et = (time.time() - t0) / k
                        ts = tick(w, "compress", ts)
                        strings, bpps = ([[], []], [[], []]), []
                        for j in range(k):
                            bj = []
                            for m_, (path, key) in enumerate(((paths[0], "r_strings"), (paths[1], "d_strings"))):
                                buf = io.BytesIO()
                                write_uints(buf, (H, Wd))
                                write_body(buf, out["shape"], [[out[key][0][j]], [out[key][1][j]]])
                                data = buf.getvalue()
                                pending.append(writers.submit(write_file, os.path.join(path, names[j]), data))
                                bj.append(float(len(data)) * 8 / (H * Wd))  # = filesize * 8 / (H * W), tester_united.py:165
                                rd = io.BytesIO(data)  # decode what the file holds, not what compress() returned
                                original_size = read_uints(rd, 2)
                                st, shape = read_body(rd)
                                strings[m_][0].append(st[0][0])
                                strings[m_][1].append(st[1][0])
                            bpps.append(bj)
                        stream.synchronize()
                        ts = tick(w, "containers", ts)
                        t0 = time.time()
                        rec = net.decompress(strings[0], strings[1], shape)
                        stream.synchronize()
                        dt = (time.time() - t0) / k
                        ts = tick(w, "decompress", ts)
                        cropper = crop0 if padding_mode.find("0") != -1 else crop1
                        xr, xd = cropper(rec["x_hat"]["r"], original_size), cropper(rec["x_hat"]["d"], original_size)
                        # [k, 4] = mse, MS-SSIM of rgb then depth: two tensor ops and one library call per modality for the group
                        # (MS-SSIM used to be ~60 torch launches per image and modality -- MIOpen convolutions, whose first
                        # use from several threads at once did not come back, and whose enqueue under the GIL was most of
                        # the wall time with 8 - 16 workers)
                        mt = torch.cat([metrics_batch(xr, rgb), metrics_batch(xd, depth)], dim=1)
                        if save:  # utils/IOutils.py:101-104, tester_united.py:98-109: the conversions on the GPU, the encoding in a writer
                            r8 = xr.clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1).contiguous().cpu().numpy()
                            d8 = xd.clamp(0, 1).mul(255).byte()[:, 0].contiguous().cpu().numpy()
                            d16 = (xd * scale16)[:, 0].to(torch.int32).cpu().numpy()
                        mt = mt.cpu().tolist()
                        ts = tick(w, "metrics_fetch", ts)
                        for j, i in enumerate(u):
                            rp, rm = finish_metrics(mt[j][0], mt[j][1])
                            dp, dm = finish_metrics(mt[j][2], mt[j][3])
                            if save:
                                rb, db, nm = bpps[j][0], bpps[j][1], names[j]
                                pending.append(writers.submit(write_png, r8[j], os.path.join(rec_dir, "rgb_rec", f"{nm}_{rb:.4f}_{rp:.4f}__rec.png")))
                                pending.append(writers.submit(write_png, d8[j], os.path.join(rec_dir, "depth_rec", f"{nm}_{db:.4f}_{dp:.4f}__rec_8bit.png")))
                                pending.append(writers.submit(write_png, d16[j], os.path.join(rec_dir, "depth_rec", f"{nm}_{db:.4f}_{dp:.4f}__rec_16bit.png"), True))
                            results[i] = (names[j], H * Wd, (rp, rm, bpps[j][0], dp, dm, bpps[j][1], dt, et))
                        tick(w, "submit_writes", ts)
            except BaseException as e:  # re-raised on the caller's thread
                errs[w] = e
                for _ in range(n):  # let the decoders run out instead of blocking on the semaphore
                    ahead.release()

        threads = [threading.Thread(target=work, args=(w,)) for w in range(W)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        decoders.shutdown(wait=True)
        self.stage_seconds = {k_: round(sum(d.get(k_, 0.0) for d in stage), 4) for k_ in sorted({k2 for d in stage for k2 in d})}
        werr = None
        for f in pending:  # every file is on disk before test_model() returns (and before its clock stops)
            try:
                f.result()
            except BaseException as e:
                werr = werr or e
        writers.shutdown(wait=True)
        for nt in nets:
            nt.per_image_streams = was_per_image
        if W >= 4:
            self.net.set_tile_mode("latency")
        if blocking:
            from ._lib import set_blocking_sync

            set_blocking_sync(False)
        for e in errs + [werr]:
            if e is not None:
                raise e

    @torch.no_grad()
    def test_model(self, padding_mode="reflect0", padding=True, workers=1, batch=4):
        """workers == 1: the reference loop (one image at a time, device-wide timing brackets).  workers > 1: the pipelined
        harness (`_test_pipelined`): that many engine instances in flight (shared weights, own stream / workspace / host
        thread), each coding up to `batch` consecutive same-size images per call, decoding and file writing in their own
        threads: files, bpp and PSNR are identical, the per-image latencies then include time-sharing of the GPU, and the
        job throughput is reported as `self.job_mpx_per_s`."""
        self.net.eval()
        names = ("avg_rgb_psnr", "avg_rgb_ms_ssim", "avg_rgb_bpp", "avg_depth_psnr", "avg_depth_ms_ssim",
                 "avg_depth_bpp", "avg_deocde_time", "avg_encode_time")
        meters = {k: AverageMeter() for k in names}
        rec_dir = self.get_rec_dir(padding=padding, padding_mode=padding_mode)
        n = len(self.test_dataloader)
        results = [None] * n
        torch.cuda.synchronize()
        t_job = time.time()
        if workers <= 1:
            for i in range(n):
                results[i] = self._one_image(i, rec_dir, padding_mode)
        else:
            self._test_pipelined(results, rec_dir, padding_mode, min(workers, n, 32), batch=max(1, int(batch)))
        torch.cuda.synchronize()
        wall = time.time() - t_job
        self.job_mpx_per_s = sum(r[1] for r in results) / max(wall, 1e-9) / 1e6
        rows = []
        for i, (name, _, vals) in enumerate(results):
            rp, rm, rb, dp, dm, db, dt, et = vals
            for k, v in zip(names, vals):
                meters[k].update(v)
            self.logger_test.info(
                f"Image[{i}:{name}] | rBpp loss: {rb:.4f} | dBpp loss: {db:.4f} | rPSNR: {rp:.4f} | dPSNR: {dp:.4f} | "
                f"rMS-SSIM: {rm:.4f} | dMS-SSIM: {dm:.4f} | Encoding Latency: {et:.4f} | Decoding latency: {dt:.4f}")
            rows.append({"name": name, "rgb_bpp": rb, "depth_bpp": db, "rgb_psnr": rp, "depth_psnr": dp,
                         "enc_time": et, "dec_time": dt})
        self.logger_test.info(
            f"Epoch:[{self.epoch}] | Avg rBpp: {meters['avg_rgb_bpp'].avg:.7f} | Avg dBpp: {meters['avg_depth_bpp'].avg:.7f} | "
            f"Avg rPSNR: {meters['avg_rgb_psnr'].avg:.7f} | Avg dPSNR: {meters['avg_depth_psnr'].avg:.7f} | "
            f"Avg rMS-SSIM: {meters['avg_rgb_ms_ssim'].avg:.7f} | Avg dMS-SSIM: {meters['avg_depth_ms_ssim'].avg:.7f} | "
            f"Avg Encoding Latency: {meters['avg_encode_time'].avg:.6f} | Avg Decoding latency: {meters['avg_deocde_time'].avg:.6f}")
        self.logger_test.info("MS-SSIM: pytorch-msssim 1.0.0's published definition restated (metrics.py; cross-checked in fp64 by "
                              "oracle/msssim_ref.py) -- not part of the pinned parity set; bpp and PSNR are")
        if workers > 1:
            self.logger_test.info(f"Job throughput with {workers} images in flight: {self.job_mpx_per_s:.3f} Mpx/s (enc+dec+I/O)")
        return rows, meters


class ImageFolder:
    """One modality of a dataset root: <root>/rgb/* (channel 3) or <root>/depth/* (channel 1), sorted by file name
    (dataset/testDataset.py:14-66)."""

    def __init__(self, root, channel=3, debug=False):
        self.mode = "RGB" if channel == 3 else "L"
        split = Path(root) / ("rgb" if channel == 3 else "depth")
        if not split.is_dir():
            raise RuntimeError(f'Invalid directory "{root}"')
        self.samples = sorted(f for f in split.iterdir() if f.is_file())
        if debug:
            self.samples = self.samples[:20]

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        return load_image(self.samples[i], self.mode)[None], [os.path.splitext(self.samples[i].name)[0]]


class TesterSingle(TesterUnited):
    """testing/tester_single.py:14-170 for the single-modal models (channel 3 or 1; `playground/test.py -m ELIC`)."""

    def __init__(self, args, config=None, net=None):
        super().__init__(types_namespace_without_dataset(args), config, net)
        self.test_dataloader = ImageFolder(args.dataset, channel=args.channel, debug=self.debug) if args.dataset else None

    # tester_single.py:121-142
    def compress_one_image(self, x, stream_path, H, W, img_name):
        torch.cuda.synchronize()
        start = time.time()
        out = self.net.compress(x)
        torch.cuda.synchronize()
        enc_time = time.time() - start
        os.makedirs(stream_path, exist_ok=True)
        fn = os.path.join(stream_path, img_name)
        with Path(fn).open("wb") as f:
            write_uints(f, (H, W))
            write_body(f, out["shape"], out["strings"])
        return float(filesize(fn)) * 8 / (H * W), enc_time

    # tester_single.py:144-170
    def decompress_one_image(self, stream_path, img_name, mode="reflect0", return_mid=False):
        with Path(os.path.join(stream_path, img_name)).open("rb") as f:
            original_size = read_uints(f, 2)
            strings, shape = read_body(f)
        torch.cuda.synchronize()
        start = time.time()
        out = self.net.decompress(strings, shape)
        torch.cuda.synchronize()
        dec_time = time.time() - start
        if return_mid:  # tester_single.py:148-149: the padded x_hat and the whole result (x_hat, up1, up2, up3), not cropped
            return out["x_hat"], dec_time, out
        cropper = crop0 if mode.find("0") != -1 else crop1
        return cropper(out["x_hat"], original_size), dec_time

    # tester_single.py:45-66
    @torch.no_grad()
    def test_model(self, padding_mode="reflect0", padding=True):
        self.net.eval()
        names = ("avg_psnr", "avg_ms_ssim", "avg_bpp", "avg_deocde_time", "avg_encode_time")
        meters = {k: AverageMeter() for k in names}
        rec_dir = self.get_rec_dir(padding=padding, padding_mode=padding_mode)
        rows = []
        for i in range(len(self.test_dataloader)):
            img, name = self.test_dataloader[i]
            _, C, H, W = img.shape
            img = img.to(self.device)
            stream_path = os.path.join(rec_dir, "depth_bin" if C == 1 else "rgb_bin")
            bpp, et = self.compress_one_image(pad(img, padding_mode), stream_path, H, W, name[0])
            x_hat, dt = self.decompress_one_image(stream_path, name[0], mode=padding_mode)
            p, m = compute_metrics(x_hat, img)
            if getattr(self, "save_reconstructions", True):  # tester_single.py:68-85
                tag = f"{name[0]}_{bpp:.4f}_{p:.4f}_"
                if C == 1:
                    save_depth16(x_hat, os.path.join(rec_dir, "depth_rec", f"{tag}_rec_16bit.png"),
                                 100000 if rec_dir.find("sun") != -1 else 10000)
                    save_image(x_hat, os.path.join(rec_dir, "depth_rec", f"{tag}_rec_8bit.png"))
                else:
                    save_image(x_hat, os.path.join(rec_dir, "rgb_rec", f"{tag}_rec.png"))
            for k, v in zip(names, (p, m, bpp, dt, et)):
                meters[k].update(v)
            self.logger_test.info(f"Image[{i}:{name[0]}] | Bpp loss: {bpp:.4f} | PSNR: {p:.4f} | MS-SSIM: {m:.4f} | "
                                  f"Encoding Latency: {et:.4f} | Decoding latency: {dt:.4f}")
            rows.append({"name": name[0], "bpp": bpp, "psnr": p, "enc_time": et, "dec_time": dt})
        self.logger_test.info(
            f"Epoch:[{self.epoch}] | Avg Bpp: {meters['avg_bpp'].avg:.7f} | Avg PSNR: {meters['avg_psnr'].avg:.7f} | "
            f"Avg MS-SSIM: {meters['avg_ms_ssim'].avg:.7f} | Avg Encoding Latency: {meters['avg_encode_time'].avg:.6f} | "
            f"Avg Decoding latency: {meters['avg_deocde_time'].avg:.6f}")
        return rows, meters


def types_namespace_without_dataset(args):
    """The base constructor opens the RGB-D pair folder; the single-modal tester opens one modality itself."""
    import copy

    a = copy.copy(args)
    exp = args.experiment or TesterUnited.get_exp_name(args.dataset, args.channel, args.model, args.quality)
    a.experiment = exp
    a.dataset = None
    return a
