// wrenc_main.cpp -- the encoder as a native program with the reference's command line (main.rs:85-115).
//
//   wrenc -i in.yuv -o out.vvc --input-size 1920x1088 --output-size 1920x1088 --num-pictures 30
//         --qp 32 --max-split-depth 2 [--reconst rec.yuv]
//
// Flow of main.rs:117-402 over the two C ABIs of this repository (include/wrenc_gpu.h for the search and
// the final pass on the MI355X, include/wrenc_bitstream.h for everything written to the stream): VPS, SPS,
// PPS once; then pictures in batches (they are independent IDR pictures, main.rs:296): read Y, Cb, Cr at
// the output size, upload, search, read the record back, write picture header NAL + slice NAL, and the
// reconstruction when asked for.  Two sets of device slots and of page-locked host buffers alternate, so
// the GPU searches batch k+1 while batch k is read back and entropy coded on a pool of host threads.
// `-` is stdin / stdout.  Argument and I/O errors print `error: ...` on stderr and exit with status 0, as the
// reference does (main.rs:127-133); a failure inside the search or the stream writer (a HIP error, a level
// that overflows the rate tables, ...) is where the reference panics (block_splitter.rs:453): status 101,
// Rust's panic status, so that a truncated stream never comes with a success status.  Options the reference does not have: --batch, --threads, --device,
// --devices (several GPUs of the node, batches in turn), --bitrate KBPS [--fps N] (rate control: every batch is measured
// on the device before its search, wrenc_gpu_download_complexity, and include/wrenc_rate.h chooses its QPs -- one, or two
// adjacent ones -- for a total of KBPS * 1000 / 8 / fps bytes per picture, parameter sets included; --qp stays the
// parameter sets' QP; the bytes depend on the input and the options alone, not on --threads or timing, which is why
// --ramp-down auto, decided by the clock, runs as never), --metrics PATH (PSNR and SSIM of every picture from sums the
// device takes of the originals and the reconstruction it holds, wrenc_gpu_download_metrics: a JSON report in the shape of
// the reference's evaluation harness, and one summary line on stderr), --pad, --scale, --input-format and --hash (below), --verbose, --ramp-down auto|always|never, --tokens auto|on|off
// (how a batch comes back.  auto and on: as the residual tokens the device makes of it, wrenc_gpu_download_tokens -- the
// host then runs the CU-level syntax and the arithmetic coder only, 1.8x less host time per picture, 20x the bytes over
// PCIe -- and as the compact level record, with residual_coding on the host, when they do not fit the token pool.  off,
// or --no-tokens: always as the compact record.  Same bytes either way).  Links only against the two C ABIs: no HIP, no
// Python.
//
// --pad: --output-size may be any even size of at least 16x16.  The input holds frames of that size.  The contexts are
// created at the next multiple of the CTU size with that visible size (wrenc_gpu_set_visible_size: the device replicates
// the last column and row into the margin), and the SPS carries the conformance window.  --reconst receives frames
// cropped to --output-size and --metrics reports that rectangle.  --bitrate charges the parameter sets of the coded
// size, so its QPs are those of the padded pictures coded plainly.
//
// --scale: the input holds frames of --input-size (even, at least 16x16, within a factor of 4 of --output-size in each
// dimension) and the device resamples every picture to --output-size behind its upload (wrenc_gpu_set_source_size; the
// filter is include/wrenc_scale.h's).  Everything else is the run on the scaled pictures: --reconst receives frames of
// --output-size, --metrics reports that size and compares the reconstruction with the SCALED originals, --pad pads the
// scaled picture, --bitrate measures it.  Without --scale, --input-size is parsed and not used, as in the reference
// (main.rs:164-174).  --scale with equal sizes changes nothing.
//
// --input-format NAME: how the input's frames lie in the file, named as ffmpeg names them (include/wrenc_format.h): yuv420p
// (the default), nv12, yuv420p10le, p010le, yuv422p, yuv422p10le.  A frame is read as it is -- its size and its planes come
// from wrenc_gpu_format_layout -- and uploaded as it is (wrenc_gpu_upload_planes); the device converts it to 8-bit 4:2:0
// behind the copy and in front of the scaler.  Everything else is the run on the converted pictures: --reconst stays 8-bit
// 4:2:0 of --output-size and --metrics compares the reconstruction with the CONVERTED (and scaled) originals.
// The name may also be an RGB layout (include/wrenc_rgb.h): rgb24, bgr24, rgb0, bgr0 (rgba and bgra are aliases) or gbrp.  The
// device then makes Y'CbCr of the frames by --colorspace bt709|bt601 (default bt709) and --range tv|pc (default tv)
// (wrenc_gpu_set_source_rgb); the two options are argument errors with a YUV input.  The stream carries no VUI: what was
// chosen is not signalled in it.
//
// --reconst-format yuv420p|nv12|rgb24|bgr24|rgb0|bgr0|rgba|bgra|gbrp (with --reconst): the frames of --reconst in that format
// at --output-size, made on the device behind the search (wrenc_gpu_download_recon; include/wrenc_recon.h): the crop, the
// interleave or the conversion to RGB by --reconst-colorspace bt709|bt601 and --reconst-range tv|pc, which default to
// --colorspace and --range of an RGB input and to bt709 tv otherwise and are argument errors with a YUV reconst format.
// The batch's read-back then leaves the coded planes on the device.  Without the option the planes are read back and
// cropped here as before; --reconst-format yuv420p writes the same file; the stream never depends on these options.
//
// --hash md5|crc|checksum: every picture's slice is followed by a decoded picture hash SEI (H.274; include/wrenc_hash.h), so
// that any conforming decoder checks what it decodes against what this encoder reconstructed.  The device takes the hash
// of the reconstruction it holds (wrenc_gpu_download_hashes: the coded planes, --pad's margin included, as a decoder
// hashes them; 48 bytes a picture over the bus) and the SEI's NAL unit (wrenc_bs_write_hash_sei) is part of the picture's
// bytes: --bitrate charges it and --metrics' frame_bytes include it.  Without the option nothing is launched or written.
//
// --target-psnr DB [--max-recodes N] (not with --bitrate, --vbv-bufsize, --qp-file): every picture at the largest QP whose luma
// PSNR is at least DB (include/wrenc_rate_quality.h on wrenc_gpu_download_dist_curve and the device's metrics); the flow is
// --vbv-bufsize's: a unit's batch is flushed before the unit uploads again, and a picture the controller does not accept is
// searched again in its slot, read back and written once more.  Without the option nothing of it is launched or allocated.
// --vbv-bufsize KBIT (with --bitrate): every picture's size is bounded by a leaky bucket of KBIT * 1000 bits that fills by
// bitrate / fps bits per picture and starts full (include/wrenc_rate.h: the buffer model; the parameter sets are charged to
// picture 0, the hash SEI to its picture).  Every batch is measured by wrenc_gpu_download_rate_hist, not by its complexity,
// and every picture gets a QP of its own.  A unit's batch is flushed BEFORE that unit uploads again, so that its slots still
// hold the originals when its bytes are known: the flush walks the batch in picture order, and a picture over its
// allowance is searched again at the QP wrenc_rate_recode returns (wrenc_gpu_set_slot_qp, wrenc_gpu_encode of that one
// slot), read back and written again, up to the largest QP; one that does not fit even there is written as it is and
// counted as a violation.  Metrics, hash and --reconst of such a picture are those of its last coding.  Only the cap is
// enforced: no filler data, no HRD syntax -- the parameter sets are byte for byte what they are without the option.
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "../../../include/wrenc_bitstream.h"
#include "../../../include/wrenc_bitstream_hash.h"
#include "../../../include/wrenc_bitstream_qp.h"
#include "../../../include/wrenc_bitstream_window.h"
#include "../../../include/wrenc_gpu.h"
#include "../../../include/wrenc_rate.h"
#include "../../../include/wrenc_rate_quality.h"
#include "../../../include/wrenc_recon.h"

namespace {

[[noreturn]] void die(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fputs("error: ", stderr);
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
    va_end(ap);
    exit(0); // main.rs:132: process::exit(0) on argument and I/O errors
}

// failures of the two libraries: the reference panics there (exit status 101)
[[noreturn]] void fatal(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fputs("error: ", stderr);
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
    va_end(ap);
    fflush(nullptr);
    _exit(101);
}

bool parse_size(const char* text, int& w, int& h) {
    char tail = 0;
    return sscanf(text, "%dx%d%c", &w, &h, &tail) == 2 && w > 0 && h > 0;
}

bool read_exact(FILE* f, uint8_t* dst, size_t n) {
    size_t got = 0;
    while (got < n) {
        const size_t r = fread(dst + got, 1, n - got, f);
        if (r == 0) return false;
        got += r;
    }
    return true;
}

// A fixed set of worker threads running index ranges (the slices of one batch).
class Pool {
public:
    explicit Pool(int n) {
        for (int i = 0; i < n; ++i) threads_.emplace_back([this] { work(); });
    }
    ~Pool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (std::thread& t : threads_) t.join();
    }
    // run fn(0..count-1) on the workers; returns at once
    void start(int count, std::function<void(int)> fn) {
        std::lock_guard<std::mutex> g(m_);
        fn_ = std::move(fn);
        count_ = count;
        next_ = 0;
        done_ = 0;
        cv_.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> g(m_);
        idle_.wait(g, [this] { return done_ == count_; });
    }

private:
    void work() {
        std::unique_lock<std::mutex> g(m_);
        for (;;) {
            cv_.wait(g, [this] { return stop_ || next_ < count_; });
            if (stop_) return;
            const int i = next_++;
            g.unlock();
            fn_(i);
            g.lock();
            if (++done_ == count_) idle_.notify_all();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex m_;
    std::condition_variable cv_, idle_;
    std::function<void(int)> fn_;
    int count_ = 0, next_ = 0, done_ = 0;
    bool stop_ = false;
};

struct Options {
    const char *input = nullptr, *output = nullptr, *reconst = nullptr, *extra = nullptr, *metrics = nullptr;
    long num_pictures = -1;
    int w = 0, h = 0, qp = 26; // the coded size; ctu.rs:382 when --qp is absent
    int vis_w = 0, vis_h = 0;  // --output-size: the size of the input's and of --reconst's frames; w x h unless --pad
    bool pad = false;
    bool scale = false;
    int in_w = 0, in_h = 0;    // the size of the input's frames: --input-size with --scale, else vis_w x vis_h
    int format = 0;            // --input-format: their pixel format (wrenc_format.h), yuv420p unless given
    int rgb = -1;              // ... or their RGB layout (wrenc_rgb.h), -1: none; then --colorspace and --range say how the
    int rgb_matrix = 0, rgb_range = 0; // device makes Y'CbCr of them: bt709 | bt601, tv | pc
    int rec_format = -1;       // --reconst-format: the output format of --reconst's frames (wrenc_recon.h), made on the device by
    int rec_matrix = 0, rec_range = 0; // wrenc_gpu_download_recon; -1: none given, the planes are read back and cropped here
    int hash = -1;             // --hash: the type of the decoded picture hash SEI behind every slice (wrenc_hash.h), -1: none
    int depth = 3, batch = 64, n_threads = 8;
    bool verbose = false;
    bool tokens = true; // --tokens auto | on: batches come back as residual tokens; --tokens off, --no-tokens: as the compact record
    int ramp_mode = 0;  // --ramp-down auto (0) | always (1) | never (2)
    std::vector<int> devices;
    std::vector<int> pic_qp; // --qp-file: the QP of every picture (empty: --qp for all)
    int min_qp = 26;         // the smallest QP of the run
    double bitrate = 0, fps = 30; // --bitrate (kbit/s, 0: none) and --fps
    double vbv_bits = 0;          // --vbv-bufsize in bits (0: no buffer model)
    double target_psnr = 0;       // --target-psnr in dB of luma PSNR (0: none) and --max-recodes
    int max_recodes = 3;
};

// --qp-file: whitespace-separated integers 0..63, entry i the QP of picture i, at least one per picture
std::vector<int> read_qp_file(const char* path, long num_pictures) {
    FILE* f = fopen(path, "r");
    if (!f) die("failed to open qp file: %s: %s", path, strerror(errno));
    std::vector<int> qps;
    char tok[64];
    while (fscanf(f, "%63s", tok) == 1) {
        char* end = nullptr;
        errno = 0;
        const long v = strtol(tok, &end, 10);
        if (end == tok || *end || errno) {
            fclose(f);
            die("Invalid qp-file entry %zu: %s", qps.size(), tok);
        }
        if (v < 0 || v > 63) {
            fclose(f);
            die("qp-file entry %zu is %ld: qp must be 0..63", qps.size(), v);
        }
        qps.push_back((int)v);
    }
    fclose(f);
    if ((long)qps.size() < num_pictures) die("qp-file has %zu entries, fewer than --num-pictures %ld", qps.size(), num_pictures);
    return qps;
}

Options parse_options(int argc, char** argv) {
    Options o;
    const char *in_size = nullptr, *out_size = nullptr, *device_list = nullptr, *qp_file = nullptr, *bitrate = nullptr, *fps = nullptr, *vbv = nullptr, *target_psnr = nullptr, *max_recodes = nullptr,
               *colorspace = nullptr, *range = nullptr, *rec_colorspace = nullptr, *rec_range = nullptr;
    int device = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const auto val = [&]() -> const char* {
            if (i + 1 >= argc) die("option %s needs a value", a.c_str());
            return argv[++i];
        };
        if (a == "-i" || a == "--input") o.input = val();
        else if (a == "-o" || a == "--output") o.output = val();
        else if (a == "-r" || a == "--reconst") o.reconst = val();
        else if (a == "--input-size") in_size = val();
        else if (a == "--output-size") out_size = val();
        else if (a == "--num-pictures") o.num_pictures = atol(val());
        else if (a == "--qp") o.qp = atoi(val());
        else if (a == "--qp-file") qp_file = val();
        else if (a == "--bitrate") bitrate = val();
        else if (a == "--fps") fps = val();
        else if (a == "--vbv-bufsize") vbv = val();
        else if (a == "--target-psnr") target_psnr = val();
        else if (a == "--max-recodes") max_recodes = val();
        else if (a == "--max-split-depth") o.depth = atoi(val());
        else if (a == "--extra-params") o.extra = val();
        else if (a == "--batch") o.batch = atoi(val());
        else if (a == "--threads") o.n_threads = atoi(val());
        else if (a == "--device") device = atoi(val());
        else if (a == "--devices") device_list = val();
        else if (a == "--metrics") o.metrics = val();
        else if (a == "--verbose") o.verbose = true;
        else if (a == "--pad") o.pad = true;
        else if (a == "--scale") o.scale = true;
        else if (a == "--input-format") {
            const char* v = val();
            o.format = wrenc_gpu_format_from_name(v);
            o.rgb = -1;
            if (o.format < 0) { // not one of the six formats: an RGB layout (include/wrenc_rgb.h)
                o.format = 0;
                o.rgb = wrenc_gpu_rgb_from_name(v);
                if (o.rgb < 0)
                    die("Invalid input-format: %s (yuv420p, nv12, yuv420p10le, p010le, yuv422p, yuv422p10le; rgb24, bgr24, rgb0, bgr0, rgba, bgra, gbrp)", v);
            }
        }
        else if (a == "--colorspace") {
            colorspace = val();
            o.rgb_matrix = !strcmp(colorspace, "bt709") ? 0 : (!strcmp(colorspace, "bt601") ? 1 : -1);
            if (o.rgb_matrix < 0) die("Invalid colorspace: %s (bt709, bt601)", colorspace);
        }
        else if (a == "--range") {
            range = val();
            o.rgb_range = !strcmp(range, "tv") ? 0 : (!strcmp(range, "pc") ? 1 : -1);
            if (o.rgb_range < 0) die("Invalid range: %s (tv, pc)", range);
        }
        else if (a == "--reconst-format") {
            const char* v = val();
            o.rec_format = wrenc_gpu_recon_from_name(v);
            if (o.rec_format < 0) die("Invalid reconst-format: %s (yuv420p, nv12; rgb24, bgr24, rgb0, bgr0, rgba, bgra, gbrp)", v);
        }
        else if (a == "--reconst-colorspace") {
            rec_colorspace = val();
            o.rec_matrix = !strcmp(rec_colorspace, "bt709") ? 0 : (!strcmp(rec_colorspace, "bt601") ? 1 : -1);
            if (o.rec_matrix < 0) die("Invalid reconst-colorspace: %s (bt709, bt601)", rec_colorspace);
        }
        else if (a == "--reconst-range") {
            rec_range = val();
            o.rec_range = !strcmp(rec_range, "tv") ? 0 : (!strcmp(rec_range, "pc") ? 1 : -1);
            if (o.rec_range < 0) die("Invalid reconst-range: %s (tv, pc)", rec_range);
        }
        else if (a == "--hash") {
            const std::string v = val();
            o.hash = v == "md5" ? WRENC_HASH_MD5 : (v == "crc" ? WRENC_HASH_CRC : (v == "checksum" ? WRENC_HASH_CHECKSUM : -1));
            if (o.hash < 0) die("Invalid hash: %s (md5, crc, checksum)", v.c_str());
        }
        else if (a == "--no-tokens") o.tokens = false;
        else if (a == "--ramp-down") { // how a run ends: auto (smaller last batches when the host's tail is heavy), always, never
            const std::string v = val();
            o.ramp_mode = v == "always" ? 1 : (v == "never" ? 2 : (v == "auto" ? 0 : -1));
            if (o.ramp_mode < 0) die("Invalid ramp-down: %s (auto, always, never)", v.c_str());
        }
        else if (a == "--tokens") {
            const std::string v = val();
            if (v != "auto" && v != "on" && v != "off") die("Invalid tokens: %s (auto, on, off)", v.c_str());
            o.tokens = v != "off";
        }
        else die("unknown option %s", a.c_str());
    }
    if (!o.input || !o.output || !in_size || !out_size || o.num_pictures < 0)
        die("the following options are required: --input --output --input-size --output-size --num-pictures");
    if ((colorspace || range) && o.rgb < 0)
        die("%s needs an RGB --input-format (rgb24, bgr24, rgb0, bgr0, rgba, bgra, gbrp): a YUV input is not converted", colorspace ? "--colorspace" : "--range");
    if (o.rec_format >= 0 && !o.reconst) die("--reconst-format needs --reconst: it is the format of that file's frames");
    if ((rec_colorspace || rec_range) && !wrenc_recon_is_rgb(o.rec_format))
        die("%s needs an RGB --reconst-format (rgb24, bgr24, rgb0, bgr0, rgba, bgra, gbrp): a YUV reconstruction is not converted",
            rec_colorspace ? "--reconst-colorspace" : "--reconst-range");
    // the way back is the way in unless said otherwise: an RGB input's matrix and range, else bt709 tv
    if (!rec_colorspace) o.rec_matrix = o.rgb >= 0 ? o.rgb_matrix : 0;
    if (!rec_range) o.rec_range = o.rgb >= 0 ? o.rgb_range : 0;
    int iw = 0, ih = 0;
    if (!parse_size(in_size, iw, ih)) die("Invalid input-size: %s", in_size); // used with --scale only (below); otherwise parsed and unused, as in main.rs:164-174
    if (!parse_size(out_size, o.w, o.h)) die("Invalid output-size: %s", out_size);
    if (o.extra) {
        const std::string e = o.extra;
        size_t pos = 0;
        while (pos <= e.size()) {
            const size_t end = e.find(',', pos) == std::string::npos ? e.size() : e.find(',', pos);
            const std::string item = e.substr(pos, end - pos);
            if (item.find('=') == std::string::npos || item.find('=') != item.rfind('='))
                die("Invalid extra-params: %s", o.extra);
            pos = end + 1;
        }
    }
    o.vis_w = o.w;
    o.vis_h = o.h;
    if (o.pad) { // any even size: coded at the next multiple of the CTU size
        if (o.w % 2 || o.h % 2 || o.w < 16 || o.h < 16) die("with --pad, output-size must be even and at least 16x16: %dx%d", o.w, o.h);
        o.w = (o.w + 31) / 32 * 32;
        o.h = (o.h + 31) / 32 * 32;
    }
    if (o.w % 32 || o.h % 32) die("output-size must be a multiple of the 32x32 CTU (picture.rs:178-181): %dx%d", o.w, o.h);
    o.in_w = o.vis_w;
    o.in_h = o.vis_h;
    if (o.scale) { // the input's frames are --input-size; the device resamples them to --output-size
        if (iw % 2 || ih % 2 || iw < 16 || ih < 16) die("with --scale, input-size must be even and at least 16x16: %dx%d", iw, ih);
        if (iw > 4 * o.vis_w || o.vis_w > 4 * iw || ih > 4 * o.vis_h || o.vis_h > 4 * ih)
            die("with --scale, input-size and output-size must be within a factor of 4 of each other: %dx%d to %dx%d", iw, ih, o.vis_w, o.vis_h);
        o.in_w = iw;
        o.in_h = ih;
    }
    if (o.qp < 0 || o.qp > 63 || o.depth < 0 || o.depth > 3) die("qp must be 0..63, max-split-depth 0..3");
    o.min_qp = o.qp;
    const auto positive = [](const char* text, double& v) { // a finite number > 0 and nothing after it
        char* end = nullptr;
        v = strtod(text, &end);
        return end != text && !*end && std::isfinite(v) && v > 0;
    };
    if (fps && !positive(fps, o.fps)) die("Invalid fps: %s", fps);
    if (bitrate) {
        if (qp_file) die("--bitrate and --qp-file exclude each other: the QPs come from the rate control or from the file");
        if (!positive(bitrate, o.bitrate)) die("Invalid bitrate: %s (kbit/s, a number above 0)", bitrate);
        o.ramp_mode = 2; // (auto looks at the clock: the batches, and with them the QPs, must not depend on it)
    }
    if (vbv) {
        if (qp_file) die("--vbv-bufsize and --qp-file exclude each other: the buffer model chooses the QPs");
        if (!bitrate) die("--vbv-bufsize needs --bitrate: the buffer fills at that rate");
        double kbit = 0;
        if (!positive(vbv, kbit)) die("Invalid vbv-bufsize: %s (kbit, a number above 0)", vbv);
        o.vbv_bits = kbit * 1000.0;
        if (o.vbv_bits < o.bitrate * 1000.0 / o.fps)
            die("vbv-bufsize %s kbit is smaller than one picture's share of the bitrate, %.3f kbit", vbv, o.bitrate / o.fps);
    }
    if (target_psnr) {
        if (bitrate || vbv || qp_file) die("--target-psnr excludes --bitrate, --vbv-bufsize and --qp-file: the QPs come from the quality target");
        if (!positive(target_psnr, o.target_psnr)) die("Invalid target-psnr: %s (dB of luma PSNR, a number above 0)", target_psnr);
        o.ramp_mode = 2; // (auto looks at the clock: the batches, and with them the QPs, must not depend on it)
    }
    if (max_recodes) {
        if (!target_psnr) die("--max-recodes needs --target-psnr");
        char* end = nullptr;
        const long v = strtol(max_recodes, &end, 10);
        if (end == max_recodes || *end || v < 0 || v > WRENC_QUALITY_MAX_RECODES) die("Invalid max-recodes: %s (0 .. %d)", max_recodes, WRENC_QUALITY_MAX_RECODES);
        o.max_recodes = (int)v;
    }
    if (qp_file) {
        o.pic_qp = read_qp_file(qp_file, o.num_pictures);
        o.pic_qp.resize((size_t)o.num_pictures);
        if (!o.pic_qp.empty()) o.min_qp = 63;
        for (int q : o.pic_qp) o.min_qp = q < o.min_qp ? q : o.min_qp;
    }
    if (o.batch < 1) o.batch = 1;
    if (o.num_pictures > 0 && o.batch > o.num_pictures) o.batch = (int)o.num_pictures;
    if (o.n_threads < 1) o.n_threads = 1;
    if (device_list) { // "0,1,2,3": HIP device ordinals, one context each (an ordinal may repeat)
        for (const char* p = device_list; *p;) {
            char* end = nullptr;
            const long d = strtol(p, &end, 10);
            if (end == p || d < 0 || (*end && *end != ',')) die("Invalid devices: %s", device_list);
            o.devices.push_back((int)d);
            p = *end ? end + 1 : end;
        }
    }
    if (o.devices.empty()) o.devices.push_back(device);
    return o;
}

// sizes of one picture (8-bit 4:2:0), of a frame of the input (in its own format) and of what is read back of a picture
struct Geometry {
    int w, h;               // the coded size
    int vw, vh;             // the size of the frames in --reconst (--pad: smaller than the coded size)
    int iw, ih;             // the size of the frames in the input (--scale: --input-size; else vw x vh)
    size_t ysz, csz, pic;   // bytes of luma, of one chroma plane, of the picture
    struct wrenc_gpu_format_layout in; // the planes of a frame of the input as it lies in the file (wrenc_gpu_format_layout)
    size_t ipic;            // ... and its bytes
    struct wrenc_gpu_format_layout rec; // --reconst-format: the planes of a frame of --reconst (wrenc_gpu_recon_layout) ...
    size_t rpic;            // ... and its bytes; without the option the coded planes as they are read back: pic
    size_t n4, maps;        // 4x4 luma blocks; bytes of cu_log2_size | luma_mode | chroma_mode
    size_t mask_words, level_blocks, n_ctus;
    Geometry(int w_, int h_, int vw_, int vh_, int iw_, int ih_, int format, int rgb, int rec_format)
        : w(w_), h(h_), vw(vw_), vh(vh_), iw(iw_), ih(ih_), ysz((size_t)w_ * h_), csz(ysz / 4), pic(ysz + 2 * csz), in(), ipic(0),
          rec(), rpic(pic), n4(ysz / 16), maps(2 * n4 + ysz / 64), mask_words(wrenc_gpu_compact_mask_words(w_, h_)), level_blocks(pic / 16),
          n_ctus((size_t)(w_ / 32) * (h_ / 32)) {
        if (rgb >= 0 ? wrenc_gpu_rgb_layout(rgb, iw_, ih_, &in) : wrenc_gpu_format_layout(format, iw_, ih_, &in)) die("input frames must be of an even size, at least 16x16: %dx%d", iw_, ih_);
        ipic = in.frame_bytes;
        if (rec_format >= 0) {
            if (wrenc_gpu_recon_layout(rec_format, vw_, vh_, &rec)) die("--reconst-format needs frames of an even size, at least 16x16: %dx%d", vw_, vh_);
            rpic = rec.frame_bytes;
        }
    }
};

struct HostSet { // one (device, slot set) unit: page-locked planes of one batch
    wrenc_gpu_ctx* ctx = nullptr;
    int base = 0;               // first slot of the set in its context
    uint8_t* in = nullptr;      // batch x (Y | Cb | Cr)
    uint8_t* rec = nullptr;     // batch x (Y | Cb | Cr), only with --reconst
    int16_t* lev = nullptr;     // batch x room for every 4x4 block of levels; the compact read-back fills the coded ones
    uint32_t* mask = nullptr;   // batch x mask of coded 4x4 blocks (wrenc_gpu_download_compact)
    std::vector<wrenc_gpu_compact> cps;
    uint32_t* tok_pool = nullptr;   // token read-back (wrenc_gpu_download_tokens): the pages of the batch; NULL: none
    size_t tok_cap = 0, tok_used = 0;
    uint32_t* tok_first = nullptr;  // batch x CTUs: first page of every CTU
    std::vector<wrenc_gpu_tokens> tks;
    bool bs_tokens = false; // the batch being written was read back as tokens
    std::atomic<long long> busy_ns{0}; // worker time spent on the batch being written
    uint8_t* maps = nullptr;    // batch x (cu_log2_size | luma_mode | chroma_mode)
    std::vector<std::vector<uint8_t>> nal; // per picture
    std::vector<int> status;
    std::vector<size_t> len;
    std::vector<wrenc_gpu_metrics> metrics; // --metrics: the batch's sums
    std::vector<wrenc_picture_hash> hashes; // --hash: the batch's hashes, until its slices are written
    int count = 0, first_poc = 0;       // the batch being searched / read back in this set
    int bs_count = 0, bs_first_poc = 0; // the batch whose slices are being written from this set
};

void gpu_check(const HostSet& s, int rc) {
    if (rc) fatal("%s", wrenc_gpu_last_error(s.ctx));
}

// the buffers of the compact level record, allocated on first use
void prepare_compact(HostSet& s, const Geometry& g, int batch) {
    if (s.lev) return;
    s.lev = (int16_t*)wrenc_gpu_alloc_host(s.ctx, g.pic * batch * sizeof(int16_t));
    s.mask = (uint32_t*)wrenc_gpu_alloc_host(s.ctx, g.mask_words * sizeof(uint32_t) * batch);
    if (!s.lev || !s.mask) fatal("%s", wrenc_gpu_last_error(s.ctx));
    s.cps.resize((size_t)batch);
}

// Words of a unit's token pool: what textured content takes at this QP (4-byte tokens per luma sample: ~1 at QP 32, ~3 at
// QP 22) with a margin; a batch that needs more is read back as the compact level record instead.  WRENC_TOKEN_POOL_WORDS
// (a test hook) replaces the estimate: that many words in whole pages, one page at least.
size_t token_pool_words(const Geometry& g, int qp, int batch) {
    const size_t page = WRENC_GPU_TOKEN_PAGE;
    if (const char* words = getenv("WRENC_TOKEN_POOL_WORDS")) {
        const size_t n = strtoull(words, nullptr, 10) / page * page;
        return n > page ? n : page;
    }
    const double per_sample = qp >= 30 ? 1.5 : (qp >= 25 ? 2.5 : 4.5);
    return (size_t)((double)g.ysz * batch * per_sample) / page * page + page * 1024;
}

// One context per entry of --devices.  Every context gets two sets of slots; a (device, set) pair is a "unit", and
// batches go to the units in turn: d0/s0, d1/s0, .., d0/s1, d1/s1, .. so that consecutive batches run on different GPUs
// and every GPU always has a batch queued behind the one it is searching.  Pictures are independent IDRs (main.rs:296):
// no data moves between GPUs.
std::vector<HostSet> make_units(const Options& o, const Geometry& g, const std::vector<wrenc_gpu_ctx*>& ctxs, int per_dev, bool with_rec) {
    const size_t n_dev = ctxs.size(), batch = (size_t)o.batch;
    std::vector<HostSet> units((size_t)per_dev * n_dev);
    for (size_t u = 0; u < units.size(); ++u) {
        HostSet& s = units[u];
        s.ctx = ctxs[u % n_dev];
        s.base = (int)(u / n_dev) * o.batch;
        s.in = (uint8_t*)wrenc_gpu_alloc_host(s.ctx, g.ipic * batch);
        s.maps = (uint8_t*)wrenc_gpu_alloc_host(s.ctx, g.maps * batch);
        if (with_rec) s.rec = (uint8_t*)wrenc_gpu_alloc_host(s.ctx, g.rpic * batch);
        if (!s.in || !s.maps || (with_rec && !s.rec)) fatal("%s", wrenc_gpu_last_error(s.ctx));
        if (o.tokens) {
            s.tok_cap = token_pool_words(g, o.min_qp, o.batch);
            s.tok_pool = (uint32_t*)wrenc_gpu_alloc_host(s.ctx, s.tok_cap * sizeof(uint32_t));
            s.tok_first = (uint32_t*)wrenc_gpu_alloc_host(s.ctx, g.n_ctus * sizeof(uint32_t) * batch);
            s.tks.resize(batch);
        }
        if (!s.tok_pool || !s.tok_first) { // --tokens off, or no page-locked memory for the pool: the compact record
            if (o.tokens && o.verbose)
                fprintf(stderr, "unit %zu: no page-locked token pool (%s), read back as the compact level record\n", u,
                        wrenc_gpu_last_error(s.ctx));
            wrenc_gpu_free_host(s.ctx, s.tok_pool);
            wrenc_gpu_free_host(s.ctx, s.tok_first);
            s.tok_pool = s.tok_first = nullptr;
            prepare_compact(s, g, o.batch);
        }
        s.nal.resize(batch);
        s.status.assign(batch, 0);
        s.len.assign(batch, 0);
        if (o.metrics) s.metrics.resize(batch);
        if (o.hash >= 0) s.hashes.resize(batch);
    }
    return units;
}

// The steps a batch goes through: read + upload + search (submit), read-back (read_back), its slices on the host threads
// (start_slices, write_picture), out in picture order (flush).
struct Run {
    const Options& o;
    const Geometry& g;
    FILE *fin, *fout, *frec;
    const int per_dev;
    // A regular input file is read by several threads at once (pread at picture offsets): one thread copies a picture of
    // 3 MB out of the page cache in about a millisecond, and the first batch's read is the one part of the run that
    // nothing overlaps.  A pipe is read in order by this thread.
    const bool seekable;
    const int n_readers;
    Pool pool;
    long poc = 0;               // the next picture to read
    long pictures = 0;          // pictures written
    unsigned long long bytes = 0;
    std::vector<wrenc_gpu_metrics> pic_metrics; // --metrics: every picture's sums and the bytes of its NAL units
    std::vector<size_t> pic_bytes;
    bool tail_heavy = false;    // writing a batch's slices keeps the threads busy for more than 0.4 of the batch's turn

    Run(const Options& o_, const Geometry& g_, FILE* in, FILE* out, FILE* rec, int per_dev_)
        : o(o_), g(g_), fin(in), fout(out), frec(rec), per_dev(per_dev_),
          seekable(fin != stdin && lseek(fileno(fin), 0, SEEK_CUR) != (off_t)-1),
          n_readers(seekable ? (o.n_threads < 8 ? o.n_threads : 8) : 1), pool(o.n_threads) {}

    // the config of every QP in use other than --qp (indexed by QP), resolved as the contexts' config was: --qp-file's by
    // main(), --bitrate's when the rate control first chooses the QP
    std::vector<const wrenc_gpu_config*> qcfg = std::vector<const wrenc_gpu_config*>(64, nullptr);
    std::vector<wrenc_gpu_config> qcfg_store;

    const wrenc_gpu_config* config_of(int q) {
        if (q == o.qp || qcfg[(size_t)q]) return qcfg[(size_t)q];
        if (qcfg_store.empty()) qcfg_store.resize(64);
        wrenc_gpu_config& c = qcfg_store[(size_t)q];
        if (wrenc_gpu_default_config(&c, o.w, o.h, q, o.depth)) fatal("%s", wrenc_gpu_last_error(nullptr));
        if (o.extra && wrenc_gpu_config_extra_params(&c, o.extra)) fatal("%s", wrenc_gpu_last_error(nullptr));
        return qcfg[(size_t)q] = &c;
    }

    // --bitrate: the controller, the QP it chose for every picture so far (sized once: the slice threads read it), and
    // the batch whose slices are being written (flushed, and so reported, before the next batch's QPs are chosen)
    wrenc_rate* rate = nullptr;
    std::vector<int> rate_qp;
    std::vector<wrenc_gpu_complexity> cplx;
    std::vector<uint64_t> rate_words;
    HostSet* pending = nullptr;
    // --vbv-bufsize: the batch's histograms; per picture the bits left in the bucket once it is taken out (negative: a
    // violation) and how often it was coded again; the run's counts
    std::vector<wrenc_rate_hist> hists;
    std::vector<double> vbv_left;
    std::vector<int> vbv_recodes;
    long vbv_reencoded = 0, vbv_violations = 0;
    // --target-psnr: a controller per unit (a unit's batch is chosen while the other unit's is still to be reported; each
    // learns from its own batches, in an order that the options alone decide), the batch's curves, every picture's codings
    // and the run's counts
    std::vector<std::pair<const HostSet*, wrenc_quality*>> quality;
    int quality_qp_max = 63;
    std::vector<wrenc_dist_curve> curves;
    std::vector<int> quality_tries;
    long quality_reencoded = 0, quality_misses = 0;

    wrenc_quality* quality_of(const HostSet& s) {
        for (const auto& q : quality)
            if (q.first == &s) return q.second;
        wrenc_quality* q = wrenc_quality_create(o.target_psnr, 0, quality_qp_max, o.max_recodes);
        if (!q) fatal("quality control: bad configuration");
        quality.emplace_back(&s, q);
        return q;
    }

    int slice_qp(long picture) const { return rate || o.target_psnr > 0 ? rate_qp[(size_t)picture] : (o.pic_qp.empty() ? o.qp : o.pic_qp[(size_t)picture]); }

    // The QPs of the unit's uploaded batch: measured on the device while the other unit's search keeps it busy, chosen
    // with every byte count known by now, set slot by slot.
    void choose_qps(HostSet& s) {
        if (o.target_psnr > 0) { // the unit's previous batch is out already (main)
            curves.resize((size_t)s.count);
            gpu_check(s, wrenc_gpu_download_dist_curve(s.ctx, s.base, s.count, curves.data()));
            std::vector<int32_t> qps((size_t)s.count);
            if (wrenc_quality_choose(quality_of(s), s.count, curves.data(), o.w, o.h, qps.data())) fatal("quality control: choose failed");
            int lo = 63, hi = 0;
            for (int k = 0; k < s.count; ++k) {
                rate_qp[(size_t)(poc + k)] = qps[(size_t)k];
                gpu_check(s, wrenc_gpu_set_slot_qp(s.ctx, s.base + k, config_of(qps[(size_t)k])));
                lo = qps[(size_t)k] < lo ? qps[(size_t)k] : lo;
                hi = qps[(size_t)k] > hi ? qps[(size_t)k] : hi;
            }
            if (o.verbose) fprintf(stderr, "  batch at picture %ld: QP %d .. %d (a QP per picture)\n", poc, lo, hi);
            return;
        }
        if (o.vbv_bits > 0) { // the unit's previous batch is out already (main): nothing to flush here
            hists.resize((size_t)s.count);
            gpu_check(s, wrenc_gpu_download_rate_hist(s.ctx, s.base, s.count, hists.data()));
            std::vector<int32_t> qps((size_t)s.count);
            if (wrenc_rate_choose_vbv(rate, s.count, hists.data(), qps.data(), nullptr)) fatal("rate control: choose failed");
            int lo = 63, hi = 0;
            for (int k = 0; k < s.count; ++k) {
                rate_qp[(size_t)(poc + k)] = qps[(size_t)k];
                gpu_check(s, wrenc_gpu_set_slot_qp(s.ctx, s.base + k, config_of(qps[(size_t)k])));
                lo = qps[(size_t)k] < lo ? qps[(size_t)k] : lo;
                hi = qps[(size_t)k] > hi ? qps[(size_t)k] : hi;
            }
            if (o.verbose) fprintf(stderr, "  batch at picture %ld: QP %d .. %d (a QP per picture)\n", poc, lo, hi);
            return;
        }
        cplx.assign((size_t)s.count, wrenc_gpu_complexity{});
        gpu_check(s, wrenc_gpu_download_complexity(s.ctx, s.base, s.count, cplx.data()));
        if (pending) {
            flush(*pending);
            pending = nullptr;
        }
        rate_words.resize((size_t)s.count * 3);
        for (int k = 0; k < s.count; ++k)
            for (int p = 0; p < 3; ++p) rate_words[(size_t)(3 * k + p)] = cplx[(size_t)k].satd[p];
        std::vector<int32_t> qps((size_t)s.count);
        if (wrenc_rate_choose(rate, s.count, rate_words.data(), qps.data())) fatal("rate control: choose failed");
        for (int k = 0; k < s.count; ++k) {
            rate_qp[(size_t)(poc + k)] = qps[(size_t)k];
            gpu_check(s, wrenc_gpu_set_slot_qp(s.ctx, s.base + k, config_of(qps[(size_t)k])));
        }
        if (o.verbose) fprintf(stderr, "  batch at picture %ld: QP %d .. %d\n", poc, (int)qps.front(), (int)qps.back());
    }

    void upload(HostSet& s, int k) {
        // the slot's QP first: the encode call of the batch reads it (NULL: the context's, --qp)
        if (!o.pic_qp.empty()) gpu_check(s, wrenc_gpu_set_slot_qp(s.ctx, s.base + k, qcfg[(size_t)slice_qp(poc + k)]));
        const uint8_t* p = s.in + g.ipic * k;
        const void* const plane[3] = {p + g.in.offset[0], p + g.in.offset[1], p + g.in.offset[2]};
        gpu_check(s, wrenc_gpu_upload_planes(s.ctx, s.base + k, plane, g.in.row_bytes));
        ++s.count;
    }

    // read + upload the next batch into the unit's slots and start its search (asynchronous)
    void submit(HostSet& s) {
        s.count = 0;
        s.first_poc = (int)poc;
        // The last batch's read-back and entropy coding overlap with nothing.  Where that is a good part of a batch's turn
        // (tail_heavy: textured content), the run ends on smaller batches -- a half, a quarter, a quarter of --batch, each a
        // little slower to search -- so that what is left at the end is a quarter's work.
        const int batch = o.batch;
        const long left = o.num_pictures - poc;
        int want = (int)(left < batch ? left : batch);
        if (per_dev == 2 && o.ramp_mode != 2 && (tail_heavy || o.ramp_mode == 1) && left <= batch && left > batch / 4) want = (int)(left / 2 > batch / 4 ? left / 2 : batch / 4);
        if (want < 1 && left > 0) want = 1;
        if (seekable && want > 0) { // (always pread then: the FILE's own position is never used)
            // readers fill the pictures (striped), this thread uploads each one as soon as it is there
            std::vector<std::atomic<int>> ready((size_t)want);
            for (auto& r : ready) r.store(0);
            std::vector<std::thread> readers;
            for (int t = 0; t < n_readers; ++t)
                readers.emplace_back([&, t] {
                    for (int k = t; k < want; k += n_readers) {
                        uint8_t* p = s.in + g.ipic * k;
                        size_t got = 0;
                        const off_t at = (off_t)((size_t)(poc + k) * g.ipic);
                        while (got < g.ipic) {
                            const ssize_t r = pread(fileno(fin), p + got, g.ipic - got, at + (off_t)got);
                            if (r <= 0) break;
                            got += (size_t)r;
                        }
                        ready[(size_t)k].store(got == g.ipic ? 1 : -1, std::memory_order_release);
                    }
                });
            int short_at = -1;
            for (int k = 0; k < want; ++k) {
                int st;
                while ((st = ready[(size_t)k].load(std::memory_order_acquire)) == 0) std::this_thread::yield();
                if (st < 0) {
                    short_at = k;
                    break;
                }
                upload(s, k);
            }
            for (std::thread& t : readers) t.join();
            if (short_at >= 0) die("input ended after %ld of %ld pictures", poc + short_at, o.num_pictures);
        } else {
            for (int k = 0; k < want; ++k) {
                if (!read_exact(fin, s.in + g.ipic * k, g.ipic)) die("input ended after %ld of %ld pictures", poc + k, o.num_pictures);
                upload(s, k);
            }
        }
        if (s.count && (rate || o.target_psnr > 0)) choose_qps(s);
        if (s.count) gpu_check(s, wrenc_gpu_encode(s.ctx, s.base, s.count));
        poc += s.count;
    }

    // The unit's batch back in ONE call (waits for its search) while the pool still writes the previous batch's slices
    // (other buffers): the residual tokens the device made of it -- the pass costs the device about 2 % of the search's
    // time and the host writes a picture 1.8 .. 2.1x faster from them -- or, when they do not fit the pool or the unit has
    // none, the compact level record (mask of coded 4x4 blocks + those blocks); either way with the maps.  True: tokens.
    bool read_back(HostSet& s) { return read_back(s, 0, s.count, s.first_poc); }

    // ... pictures k0 .. k0 + n - 1 of the unit's batch, which starts at picture first_poc (the whole batch, or the one
    // picture --vbv-bufsize has searched again: the token pool is free then, the batch's slices are written)
    bool read_back(HostSet& s, int k0, int n, int first_poc) {
        if (o.metrics) { // the slots still hold the batch's originals next to its reconstruction: their sums, 60 bytes a picture
            gpu_check(s, wrenc_gpu_download_metrics(s.ctx, s.base + k0, n, s.metrics.data() + k0));
            if (pic_metrics.size() < (size_t)(first_poc + k0 + n)) pic_metrics.resize((size_t)(first_poc + k0 + n));
            for (int k = k0; k < k0 + n; ++k) pic_metrics[(size_t)(first_poc + k)] = s.metrics[(size_t)k];
        }
        // --hash: of the reconstruction where it lies, 48 bytes a picture (the unit's slices of the batch before are out)
        if (o.hash >= 0) gpu_check(s, wrenc_gpu_download_hashes(s.ctx, s.base + k0, n, o.hash, s.hashes.data() + k0));
        // --reconst-format: the frames of --reconst as the device makes them, cropped and converted (include/wrenc_recon.h); the
        // coded planes then stay where they are
        if (frec && o.rec_format >= 0) {
            const wrenc_gpu_recon_format f = {o.rec_format, o.rec_matrix, o.rec_range};
            for (int k = k0; k < k0 + n; ++k) {
                uint8_t* frame = s.rec + g.rpic * k;
                void* const plane[3] = {frame + g.rec.offset[0], frame + g.rec.offset[1], frame + g.rec.offset[2]};
                gpu_check(s, wrenc_gpu_download_recon(s.ctx, s.base + k, &f, plane, g.rec.row_bytes));
            }
        }
        if (s.tok_pool) {
            for (int k = k0; k < k0 + n; ++k) {
                uint8_t* m = s.maps + g.maps * k;
                uint8_t* r = frec && o.rec_format < 0 ? s.rec + g.pic * k : nullptr;
                s.tks[(size_t)k] = wrenc_gpu_tokens{s.tok_first + g.n_ctus * k, m, m + g.n4, m + 2 * g.n4, r, r ? r + g.ysz : nullptr, r ? r + g.ysz + g.csz : nullptr};
            }
            const int rc = wrenc_gpu_download_tokens(s.ctx, s.base + k0, n, s.tks.data() + k0, s.tok_pool, s.tok_cap, &s.tok_used);
            if (rc == WRENC_GPU_OK) return true;
            if (rc != WRENC_GPU_ENOMEM) gpu_check(s, rc);
            if (o.verbose)
                fprintf(stderr, "batch at picture %d: more tokens than the pool holds, read back as the compact level record\n", first_poc + k0);
            prepare_compact(s, g, o.batch);
        }
        for (int k = k0; k < k0 + n; ++k) {
            uint8_t* m = s.maps + g.maps * k;
            uint8_t* r = frec && o.rec_format < 0 ? s.rec + g.pic * k : nullptr;
            s.cps[(size_t)k] = wrenc_gpu_compact{s.mask + g.mask_words * k, s.lev + g.pic * k, g.level_blocks, 0, m, m + g.n4, m + 2 * g.n4,
                                                 r, r ? r + g.ysz : nullptr, r ? r + g.ysz + g.csz : nullptr};
        }
        gpu_check(s, wrenc_gpu_download_compact(s.ctx, s.base + k0, n, s.cps.data() + k0));
        return false;
    }

    // picture k of the batch the unit writes, into s.nal[k], from the record it was read back as
    void write_picture(HostSet& s, int k) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint8_t* m = s.maps + g.maps * k;
        const int poc_k = s.bs_first_poc + k;
        wrenc_bs_tokens tk = {m, m + g.n4, m + 2 * g.n4, s.tok_pool, s.tok_cap, nullptr};
        wrenc_bs_record rec = {m, m + g.n4, m + 2 * g.n4, nullptr, nullptr, nullptr};
        if (s.bs_tokens) { // the device made the residual tokens: CU-level syntax + arithmetic coder here
            tk.first_page = s.tok_first + g.n_ctus * k;
        } else { // the level planes the stream writer reads, rebuilt from the compact record in this thread's own buffer
            static thread_local std::vector<int16_t> dense;
            if (dense.size() < g.pic) dense.resize(g.pic);
            int16_t* l = dense.data();
            wrenc_gpu_expand_levels(g.w, g.h, s.mask + g.mask_words * k, s.lev + g.pic * k, l, l + g.ysz, l + g.ysz + g.csz);
            rec.lev_y = l;
            rec.lev_cb = l + g.ysz;
            rec.lev_cr = l + g.ysz + g.csz;
        }
        std::vector<uint8_t>& out = s.nal[(size_t)k];
        const auto write = [&](size_t* n) {
            const int q = slice_qp(poc_k);
            return s.bs_tokens ? wrenc_bs_write_picture_tokens_qp(g.w, g.h, o.qp, q, poc_k, &tk, out.data(), out.size(), n)
                               : wrenc_bs_write_picture_qp(g.w, g.h, o.qp, q, poc_k, &rec, out.data(), out.size(), n);
        };
        // wrenc_bs_picture_bound is the proven worst case (12 bytes per luma sample); real pictures need a small fraction,
        // and the writer reports the size it needs when the buffer is too small
        const size_t first_guess = g.ysz / 2 + 65536;
        if (out.size() < first_guess) out.resize(first_guess);
        size_t n = 0;
        int rc = write(&n);
        if (rc == WRENC_BS_ENOSPC) {
            out.resize(n);
            rc = write(&n);
        }
        if (!rc && o.hash >= 0) { // the decoded picture hash SEI directly behind the slice: part of the picture's bytes
            size_t sei = 0;
            rc = wrenc_bs_write_hash_sei(o.hash, &s.hashes[(size_t)k], out.data() + n, out.size() - n, &sei);
            if (rc == WRENC_BS_ENOSPC) {
                out.resize(n + sei);
                rc = wrenc_bs_write_hash_sei(o.hash, &s.hashes[(size_t)k], out.data() + n, out.size() - n, &sei);
            }
            n += sei;
        }
        s.status[(size_t)k] = rc;
        s.len[(size_t)k] = rc ? 0 : n;
        s.busy_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    }

    // the slices of the unit's batch on the pool; flush() collects them in picture order
    void start_slices(HostSet& s, bool tokens) {
        s.bs_tokens = tokens;
        s.bs_count = s.count;
        s.bs_first_poc = s.first_poc;
        s.busy_ns.store(0);
        pool.start(s.count, [this, &s](int k) { write_picture(s, k); });
    }

    // a picture's reconstruction (coded size, as it is read back) to --reconst, cropped to the frames' size
    void write_reconst(const uint8_t* rec) {
        if (g.vw == g.w && g.vh == g.h) {
            fwrite(rec, 1, g.pic, frec);
            return;
        }
        for (int p = 0; p < 3; ++p) {
            const size_t pitch = (size_t)(p ? g.w / 2 : g.w), cols = (size_t)(p ? g.vw / 2 : g.vw), rows = (size_t)(p ? g.vh / 2 : g.vh);
            const uint8_t* plane = rec + (p ? g.ysz + (size_t)(p - 1) * g.csz : 0);
            for (size_t r = 0; r < rows; ++r) fwrite(plane + r * pitch, 1, cols, frec);
        }
    }

    // --vbv-bufsize: picture k of the batch being flushed against the bucket.  Over its allowance it is searched again at
    // the controller's QP while its slot still holds the originals, read back and written again on this thread, until it
    // fits or the QP is the largest; then it is reported, which moves the bucket on.
    void enforce_vbv(HostSet& s, int k) {
        const size_t picture = (size_t)(s.bs_first_poc + k);
        double allowance = 0;
        if (wrenc_rate_vbv_allowance(rate, &allowance, nullptr, nullptr)) fatal("rate control: no buffer model");
        while (!s.status[(size_t)k] && 8.0 * (double)s.len[(size_t)k] > allowance) {
            int32_t q = 0;
            if (wrenc_rate_recode(rate, s.len[(size_t)k], allowance, &q)) fatal("rate control: recode failed");
            if (q == rate_qp[picture]) break; // the largest QP already: written as it is
            rate_qp[picture] = q;
            ++vbv_recodes[picture];
            gpu_check(s, wrenc_gpu_set_slot_qp(s.ctx, s.base + k, config_of(q)));
            gpu_check(s, wrenc_gpu_encode(s.ctx, s.base + k, 1));
            const bool batch_tokens = s.bs_tokens;
            s.bs_tokens = read_back(s, k, 1, s.bs_first_poc);
            write_picture(s, k);
            s.bs_tokens = batch_tokens;
        }
        if (s.status[(size_t)k]) return; // (flush reports the failure)
        vbv_left[picture] = allowance - 8.0 * (double)s.len[(size_t)k];
        vbv_reencoded += vbv_recodes[picture] > 0;
        vbv_violations += vbv_left[picture] < 0;
        const uint64_t bytes_k = s.len[(size_t)k];
        if (wrenc_rate_report(rate, 1, &bytes_k)) fatal("rate control: report failed");
    }

    // --target-psnr: picture k of the batch being flushed against the target.  Its coding's luma SSE goes to the unit's
    // controller, which keeps it or names the QP to search it again at while its slot still holds the originals; the
    // picture is then read back and written again on this thread.  Where the coding to keep is an earlier one (a higher QP
    // fell below the target), the picture is searched once more at that QP: the same coding, nothing is kept in memory.
    void enforce_quality(HostSet& s, int k) {
        const size_t picture = (size_t)(s.bs_first_poc + k);
        wrenc_quality* q = quality_of(s);
        int codings = 1;
        while (!s.status[(size_t)k]) {
            wrenc_gpu_metrics m;
            gpu_check(s, wrenc_gpu_download_metrics(s.ctx, s.base + k, 1, &m));
            int32_t next = 0;
            int accepted = 0;
            if (wrenc_quality_report(q, k, rate_qp[picture], m.sse[0], (uint64_t)o.vis_w * (uint64_t)o.vis_h, &next, &accepted))
                fatal("quality control: report failed");
            if (accepted && next == rate_qp[picture]) break;
            rate_qp[picture] = next;
            ++codings;
            gpu_check(s, wrenc_gpu_set_slot_qp(s.ctx, s.base + k, config_of(next)));
            gpu_check(s, wrenc_gpu_encode(s.ctx, s.base + k, 1));
            const bool batch_tokens = s.bs_tokens;
            s.bs_tokens = read_back(s, k, 1, s.bs_first_poc);
            write_picture(s, k);
            s.bs_tokens = batch_tokens;
            if (accepted) break;
        }
        quality_tries[picture] = codings;
        quality_reencoded += codings - 1;
    }

    void flush(HostSet& s) {
        pool.wait();
        const long reenc0 = vbv_reencoded, viol0 = vbv_violations;
        const long q_reenc0 = quality_reencoded;
        uint64_t q_miss0 = 0, q_miss1 = 0;
        if (o.target_psnr > 0) wrenc_quality_totals(quality_of(s), nullptr, &q_miss0);
        for (int k = 0; k < s.bs_count; ++k) {
            if (o.target_psnr > 0) enforce_quality(s, k);
            if (o.vbv_bits > 0) enforce_vbv(s, k);
            if (s.status[(size_t)k]) fatal("wrenc_bs_write_picture failed with %d on picture %d", s.status[(size_t)k], s.bs_first_poc + k);
            fwrite(s.nal[(size_t)k].data(), 1, s.len[(size_t)k], fout);
            bytes += s.len[(size_t)k];
            if (o.metrics) pic_bytes.push_back(s.len[(size_t)k]);
            if (frec && o.rec_format >= 0) fwrite(s.rec + g.rpic * k, 1, g.rpic, frec);
            else if (frec) write_reconst(s.rec + g.pic * k); // main.rs:387-399
        }
        if (o.target_psnr > 0) {
            wrenc_quality_totals(quality_of(s), nullptr, &q_miss1);
            quality_misses += (long)(q_miss1 - q_miss0);
            if (o.verbose && s.bs_count > 0)
                fprintf(stderr, "  quality: batch at picture %d: %ld re-encoded, %ld misses\n", s.bs_first_poc, quality_reencoded - q_reenc0, (long)(q_miss1 - q_miss0));
        }
        if (o.vbv_bits > 0) { // (reported picture by picture, above)
            if (o.verbose && s.bs_count > 0)
                fprintf(stderr, "  vbv: batch at picture %d: %ld re-encoded, %ld violations\n", s.bs_first_poc, vbv_reencoded - reenc0, vbv_violations - viol0);
        } else if (rate && s.bs_count > 0) { // the bytes of the batch's NAL units, in the order its QPs were chosen
            rate_words.assign(s.len.begin(), s.len.begin() + s.bs_count);
            if (wrenc_rate_report(rate, s.bs_count, rate_words.data())) fatal("rate control: report failed");
        }
        pictures += s.bs_count;
    }
};

// --metrics: the report of the run in the shape of the reference's evaluation harness (metrics.json: per metric a summary and
// the frames, attributes Avg / Y / U / V), with the pictures' bytes and QPs; a summary is the mean over the frames, an
// infinite one (every frame identical) written as 100 as the harness does.  Numbers round-trip (%.17g).
void write_metrics_report(const Run& run, const char* path, unsigned long long stream_bytes) {
    const Options& o = run.o;
    const size_t n = run.pic_metrics.size();
    std::vector<double> psnr(4 * n), ssim(4 * n);
    double mean[2][4] = {};
    for (size_t i = 0; i < n; ++i) {
        wrenc_gpu_metrics_values(o.vis_w, o.vis_h, &run.pic_metrics[i], &psnr[4 * i], &ssim[4 * i]);
        for (int a = 0; a < 4; ++a) {
            mean[0][a] += psnr[4 * i + a];
            mean[1][a] += ssim[4 * i + a];
        }
    }
    for (auto& m : mean)
        for (double& v : m) {
            v = n ? v / (double)n : 0.0;
            if (std::isinf(v)) v = 100.0;
        }
    FILE* f = fopen(path, "w");
    if (!f) die("failed to open metrics file: %s", strerror(errno));
    const char* const attr[4] = {"Avg", "Y", "U", "V"};
    const auto number = [&](double v) {
        if (std::isinf(v)) fputs(v > 0 ? "Infinity" : "-Infinity", f);
        else fprintf(f, "%.17g", v);
    };
    fprintf(f, "{\"width\": %d, \"height\": %d, \"frames\": %zu", o.vis_w, o.vis_h, n);
    for (int m = 0; m < 2; ++m) {
        const std::vector<double>& v = m ? ssim : psnr;
        fprintf(f, ",\n \"%s\": {\"summary\": {", m ? "SSIM" : "PSNR");
        for (int a = 0; a < 4; ++a) {
            fprintf(f, "%s\"%s\": ", a ? ", " : "", attr[a]);
            number(mean[m][a]);
        }
        fputs("}, \"per_frame\": [", f);
        for (size_t i = 0; i < n; ++i) {
            fprintf(f, "%s\n  {\"n\": %zu", i ? "," : "", i + 1);
            for (int a = 0; a < 4; ++a) {
                fprintf(f, ", \"%s\": ", attr[a]);
                number(v[4 * i + a]);
            }
            fputc('}', f);
        }
        fputs("]}", f);
    }
    fputs(",\n \"frame_bytes\": [", f);
    for (size_t i = 0; i < run.pic_bytes.size(); ++i) fprintf(f, "%s%zu", i ? ", " : "", run.pic_bytes[i]);
    fputs("],\n \"frame_qp\": [", f);
    for (size_t i = 0; i < n; ++i) fprintf(f, "%s%d", i ? ", " : "", run.slice_qp((long)i));
    fputc(']', f);
    if (o.vbv_bits > 0) { // fullness: the bits left in the bucket once the picture is taken out, negative for a violation
        fprintf(f, ",\n \"vbv\": {\"bufsize_bits\": %.17g, \"reencoded\": %ld, \"violations\": %ld, \"fullness\": [", o.vbv_bits, run.vbv_reencoded, run.vbv_violations);
        for (size_t i = 0; i < n; ++i) fprintf(f, "%s%.17g", i ? ", " : "", run.vbv_left[i]);
        fputs("]}", f);
    }
    if (o.target_psnr > 0) {
        fprintf(f, ",\n \"quality\": {\"target_psnr\": %.17g, \"reencoded\": %ld, \"misses\": %ld, \"tries\": [", o.target_psnr, run.quality_reencoded, run.quality_misses);
        for (size_t i = 0; i < n; ++i) fprintf(f, "%s%d", i ? ", " : "", run.quality_tries[i]);
        fputs("]}", f);
    }
    fputs("}\n", f);
    fclose(f);
    fprintf(stderr, "%llu bytes  %.4f bpp  PSNR Avg %.2f Y %.2f U %.2f V %.2f dB  SSIM All %.4f Y %.4f\n", stream_bytes,
            n ? 8.0 * (double)stream_bytes / ((double)n * o.vis_w * o.vis_h) : 0.0, mean[0][0], mean[0][1], mean[0][2], mean[0][3], mean[1][0], mean[1][1]);
}

double since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
}

} // namespace

int main(int argc, char** argv) {
    // 4 encode lanes + 1 copy stream per context: more hardware queues than the HIP runtime's default of 4 let the
    // read-back overlap the search (must be in the environment before the first HIP call; an explicit setting wins)
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    const Options o = parse_options(argc, argv);
    FILE* fin = strcmp(o.input, "-") ? fopen(o.input, "rb") : stdin;
    if (!fin) die("failed to open input file: %s", strerror(errno));
    FILE* fout = strcmp(o.output, "-") ? fopen(o.output, "wb") : stdout;
    if (!fout) die("failed to open output file: %s", strerror(errno));
    FILE* frec = nullptr;
    if (o.reconst && !(frec = fopen(o.reconst, "wb"))) die("failed to open reconst file: %s", strerror(errno));

    const int n_dev = (int)o.devices.size();
    const int per_dev = o.num_pictures > (long)o.batch * n_dev ? 2 : 1;
    wrenc_gpu_config cfg;
    if (wrenc_gpu_default_config(&cfg, o.w, o.h, o.qp, o.depth)) fatal("%s", wrenc_gpu_last_error(nullptr));
    if (o.extra && wrenc_gpu_config_extra_params(&cfg, o.extra)) fatal(  // a value that is not a number: parse().unwrap() panics in the reference
       "%s", wrenc_gpu_last_error(nullptr));
    cfg.n_slots = per_dev * o.batch;
    std::vector<wrenc_gpu_ctx*> ctxs;
    for (int d : o.devices) {
        cfg.device = d;
        wrenc_gpu_ctx* ctx = nullptr;
        if (wrenc_gpu_create(&cfg, &ctx)) fatal("%s", wrenc_gpu_last_error(nullptr)); // no CPU path: fails without an MI355X
        if (o.pad && wrenc_gpu_set_visible_size(ctx, o.vis_w, o.vis_h)) fatal("%s", wrenc_gpu_last_error(ctx));
        if (o.scale && wrenc_gpu_set_source_size(ctx, o.in_w, o.in_h)) fatal("%s", wrenc_gpu_last_error(ctx)); // after the visible size
        if (o.format && wrenc_gpu_set_source_format(ctx, o.format)) fatal("%s", wrenc_gpu_last_error(ctx));
        if (o.rgb >= 0 && wrenc_gpu_set_source_rgb(ctx, o.rgb, o.rgb_matrix, o.rgb_range)) fatal("%s", wrenc_gpu_last_error(ctx));
        ctxs.push_back(ctx);
    }
    const Geometry g(o.w, o.h, o.vis_w, o.vis_h, o.in_w, o.in_h, o.format, o.rgb, o.rec_format);
    std::vector<HostSet> units = make_units(o, g, ctxs, per_dev, frec != nullptr);
    size_t hdr_bytes = 0, rate_hdr_bytes = 0;
    {
        uint8_t hdr[512];
        size_t n = 0;
        // (the visible size equal to the coded one: the bytes of wrenc_bs_write_parameter_sets)
        if (wrenc_bs_write_parameter_sets_window(o.w, o.h, o.vis_w, o.vis_h, o.qp, hdr, sizeof(hdr), &n)) fatal("parameter sets do not fit");
        fwrite(hdr, 1, n, fout);
        hdr_bytes = n;
        // --bitrate charges the parameter sets of the coded size: the byte or two of the window fields stay outside the
        // budget, so a padded run chooses exactly the QPs of a plain run over the padded pictures
        if (wrenc_bs_write_parameter_sets(o.w, o.h, o.qp, hdr, sizeof(hdr), &rate_hdr_bytes)) fatal("parameter sets do not fit");
    }

    const auto t_start = std::chrono::steady_clock::now();
    Run run(o, g, fin, fout, frec, per_dev);
    for (int q : o.pic_qp) run.config_of(q); // --qp-file: resolved as the contexts' config was
    const double target_bytes = o.bitrate * 1000.0 / 8.0 / o.fps;
    if (o.bitrate > 0 && o.num_pictures > 0) {
        // --extra-params can push the quantiser's rate model out of the device's 32-bit range at high QPs (lambda_q grows
        // with the QP: wrenc_gpu_set_slot_qp refuses those): the rate control stays below the first QP that does not fit
        int qp_max = 63;
        while (qp_max > o.qp && wrenc_gpu_set_slot_qp(ctxs[0], 0, run.config_of(qp_max)) == WRENC_GPU_EINVAL) --qp_max;
        if (wrenc_gpu_set_slot_qp(ctxs[0], 0, nullptr)) fatal("%s", wrenc_gpu_last_error(ctxs[0]));
        // (the buffer model charges the parameter sets as they are written, window fields included: its cap is on real bits)
        const wrenc_rate_config rcfg = {o.w, o.h, 0, qp_max, (int64_t)o.num_pictures, target_bytes, (double)(o.vbv_bits > 0 ? hdr_bytes : rate_hdr_bytes)};
        if (wrenc_rate_create(&rcfg, &run.rate)) fatal("rate control: bad configuration");
        if (o.vbv_bits > 0) {
            if (wrenc_rate_enable_vbv(run.rate, o.vbv_bits)) die("vbv-bufsize %.0f bits does not hold the parameter sets (%zu bytes)", o.vbv_bits, hdr_bytes);
            run.vbv_left.assign((size_t)o.num_pictures, 0.0);
            run.vbv_recodes.assign((size_t)o.num_pictures, 0);
        }
        run.rate_qp.assign((size_t)o.num_pictures, o.qp);
        if (o.verbose) fprintf(stderr, "rate control: %.1f kbit/s at %.3g pictures/s = %.1f bytes per picture, QP 0 .. %d\n", o.bitrate, o.fps, target_bytes, qp_max);
    }
    if (o.target_psnr > 0 && o.num_pictures > 0) { // (the QPs stay below the first one --extra-params pushes out of range, as above)
        while (run.quality_qp_max > o.qp && wrenc_gpu_set_slot_qp(ctxs[0], 0, run.config_of(run.quality_qp_max)) == WRENC_GPU_EINVAL) --run.quality_qp_max;
        if (wrenc_gpu_set_slot_qp(ctxs[0], 0, nullptr)) fatal("%s", wrenc_gpu_last_error(ctxs[0]));
        run.rate_qp.assign((size_t)o.num_pictures, o.qp);
        run.quality_tries.assign((size_t)o.num_pictures, 0);
        if (o.verbose) fprintf(stderr, "quality control: luma PSNR of at least %.3f dB, at most %d re-encodes a picture, QP 0 .. %d\n", o.target_psnr, o.max_recodes, run.quality_qp_max);
    }
    // Fill every unit, then go round: read the oldest batch back (waits for its search only), collect the
    // slices of the batch before it (written meanwhile), start this batch's slices, and give the unit the next
    // batch.  With --reconst the planes of a batch are written out before its unit is read back into again.
    for (HostSet& s : units)
        if (run.poc < o.num_pictures) run.submit(s);
    HostSet*& pending = run.pending;
    // --verbose: where the main thread spends the run (waiting for slices, for the search + read-back, reading + uploading)
    double t_flush = 0, t_readback = 0, t_submit = 0;
    int n_token_batches = 0;
    auto t_turn = std::chrono::steady_clock::now();
    if (o.verbose) fprintf(stderr, "first batches submitted after %.3f s\n", since(t_start));
    for (size_t head = 0; units[head].count > 0; head = (head + 1) % units.size()) {
        HostSet& s = units[head];
        auto tp = std::chrono::steady_clock::now();
        const bool tokens = run.read_back(s);
        t_readback += since(tp);
        if (o.verbose) fprintf(stderr, "  %.3f s: batch at picture %d read back (%s)", since(t_start), s.first_poc, tokens ? "tokens" : "compact");
        tp = std::chrono::steady_clock::now();
        if (pending) run.flush(*pending); // the previous batch's slices, in picture order, to the output
        if (o.verbose) fprintf(stderr, ", %.3f s: previous batch's slices out", since(t_start));
        {
            const double waited = since(tp), turn = since(t_turn);
            t_flush += waited;
            if (pending && pending->bs_count > 0 && turn > 0) run.tail_heavy = (double)pending->busy_ns.load() * 1e-9 > 0.4 * o.n_threads * turn;
            n_token_batches += tokens ? 1 : 0;
            t_turn = std::chrono::steady_clock::now();
        }
        tp = std::chrono::steady_clock::now();
        run.start_slices(s, tokens);
        pending = &s;
        s.count = 0;
        if (o.vbv_bits > 0 || o.target_psnr > 0) { // the unit's batch out, and enforced, while its slots still hold the originals
            const auto tf = std::chrono::steady_clock::now();
            run.flush(s);
            pending = nullptr;
            t_flush += since(tf);
        }
        if (run.poc < o.num_pictures) {
            if (units.size() == 1 && pending) { // a single unit: its slices must be out before its buffers are refilled
                run.flush(s);
                pending = nullptr;
            }
            run.submit(s);
        }
        t_submit += since(tp);
        if (o.verbose) fprintf(stderr, ", %.3f s: next batch submitted\n", since(t_start));
    }
    {
        const auto tp = std::chrono::steady_clock::now();
        if (pending) run.flush(*pending);
        t_flush += since(tp);
    }
    if (o.verbose)
        fprintf(stderr, "main thread: %.3f s waiting for slices, %.3f s for search + read-back, %.3f s reading + uploading; %d batch(es) read back as tokens\n",
                t_flush, t_readback, t_submit, n_token_batches);
    fflush(fout);
    if (frec) fclose(frec);
    if (fout != stdout) fclose(fout);
    if (o.metrics) write_metrics_report(run, o.metrics, run.bytes + hdr_bytes);
    if (o.vbv_bits > 0) fprintf(stderr, "vbv: %ld re-encoded, %ld violations\n", run.vbv_reencoded, run.vbv_violations);
    if (o.verbose && run.rate && run.pictures > 0) {
        const double total = (double)(run.bytes + hdr_bytes), want = target_bytes * (double)run.pictures;
        fprintf(stderr, "rate control: target %.1f kbit/s, achieved %.1f kbit/s (%.0f of %.0f bytes, ratio %.4f)\n", o.bitrate,
                total / (double)run.pictures * 8.0 * o.fps / 1000.0, total, want, total / want);
    }
    if (o.target_psnr > 0) fprintf(stderr, "quality: %ld re-encoded, %ld misses\n", run.quality_reencoded, run.quality_misses);
    for (const auto& q : run.quality) wrenc_quality_destroy(q.second);
    wrenc_rate_destroy(run.rate);
    if (o.verbose) {
        const double dt = since(t_start);
        fprintf(stderr, "%ld pictures, %llu bytes, %.2f s, %.1f pictures/s (file to stream, %d GPU context(s), %d host threads)\n",
                run.pictures, run.bytes, dt, run.pictures / (dt > 0 ? dt : 1e-9), n_dev, o.n_threads);
    }
    for (HostSet& s : units) {
        wrenc_gpu_free_host(s.ctx, s.in);
        wrenc_gpu_free_host(s.ctx, s.lev);
        wrenc_gpu_free_host(s.ctx, s.maps);
        wrenc_gpu_free_host(s.ctx, s.mask);
        wrenc_gpu_free_host(s.ctx, s.tok_pool);
        wrenc_gpu_free_host(s.ctx, s.tok_first);
        wrenc_gpu_free_host(s.ctx, s.rec);
    }
    for (wrenc_gpu_ctx* ctx : ctxs) wrenc_gpu_destroy(ctx);
    return 0;
}
