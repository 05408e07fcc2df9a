// quadrs-hip — the reference's CLI operator chain (from / gen / shift / lowpass / sparkfft / bucket /
// write) driven through the C ABI of the MI355X engine (include/quadrs_hip.h).
//
// Host glue only: the grammar and defaults restate src/args.rs, the chain plumbing restates
// Operation::exec (src/lib.rs:83-175) and the Samples iterator (src/samples.rs:11-28).  Every
// sample-touching step is a call into libquadrs_hip.so; there is no CPU arithmetic path here.
// stdout is byte-identical to the reference's for the same command line; diagnostics go to stderr.
//
// Chains of the shape  from|gen [shift] [lowpass]  ->  sparkfft|bucket  run as ONE fused plan
// (qd_plan_*); other shift / lowpass stage lists in front of sparkfft|bucket (a shift after the filter, two cascaded
// lowpasses) go to a fused cascade plan (qd_plan_create_stages), in front of write too.  Anything else (e.g. three lowpasses)
// falls back to the block iterator, whose read_at() calls the fine-grained entry points exactly where the reference's read_at()
// computes.
#include <algorithm>
#include <functional>
#include <cerrno>
#include <cmath>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <map>
#include <memory>
#include <regex>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

#include "../../include/quadrs_hip.h"

namespace {

struct Fail { std::string msg; };
[[noreturn]] void bail(const std::string &m) { throw Fail{m}; }
void qd_check(int rc, const char *what) {
    if (rc != QD_OK) bail(std::string(what) + ": " + qd_last_error() + (rc == QD_ERR_PANIC ? " (the reference panics here)" : ""));
}

// ------------------------------------------------------------------ src/args.rs

// find_multiplication_suffix + parse_si_*  (src/args.rs:335-379)
bool split_si(const std::string &from, std::string &val, uint64_t &mul) {
    mul = 1; val = from;
    if (from.empty()) return true;
    switch (from.back()) {
    case 'k': mul = 1000ull; break;
    case 'M': mul = 1000000ull; break;
    case 'G': mul = 1000000000ull; break;
    default: return true;
    }
    val = from.substr(0, from.size() - 1);
    return true;
}
uint64_t parse_si_u64(const std::string &s) {
    std::string v; uint64_t mul; split_si(s, v, mul);
    if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos) bail("invalid digit found in string: " + s);
    errno = 0;
    unsigned long long p = strtoull(v.c_str(), nullptr, 10);
    if (errno) bail("number too large: " + s);
    unsigned __int128 r = (unsigned __int128)p * mul;
    if (r > UINT64_MAX) bail("unit is out of range: " + s);
    return (uint64_t)r;
}
int64_t parse_si_i64(const std::string &s) {
    std::string v; uint64_t mul; split_si(s, v, mul);
    size_t start = (!v.empty() && (v[0] == '-' || v[0] == '+')) ? 1 : 0;
    if (v.size() == start || v.find_first_not_of("0123456789", start) != std::string::npos) bail("invalid digit found in string: " + s);
    errno = 0;
    long long p = strtoll(v.c_str(), nullptr, 10);
    if (errno) bail("number too large: " + s);
    __int128 r = (__int128)p * (__int128)mul;
    if (r > INT64_MAX || r < INT64_MIN) bail("unit is out of range: " + s);
    return (int64_t)r;
}
double parse_si_f64(const std::string &s) {
    std::string v; uint64_t mul; split_si(s, v, mul);
    char *end = nullptr;
    double p = strtod(v.c_str(), &end);
    if (v.empty() || *end) bail("invalid float literal: " + s);
    return p * (double)mul;
}
bool parse_bool(const std::string &s) {       // src/args.rs:381-390
    if (s == "true" || s == "yes" || s == "y") return true;
    if (s == "false" || s == "no" || s == "n") return false;
    bail("unacceptable boolean value: '" + s + "'");
}

// guess_from_extension (src/args.rs:392-402)
int format_from_ext(const std::string &ext) {
    if (ext == "cf32" || ext == "fc32") return QD_FMT_CF32;
    if (ext == "cs8" || ext == "sc8" || ext == "c8") return QD_FMT_CS8;
    if (ext == "cu8" || ext == "su8") return QD_FMT_CU8;
    if (ext == "cs16" || ext == "sc16" || ext == "c16") return QD_FMT_CS16;
    return -1;
}

enum OpKind { OP_FROM, OP_GEN, OP_SHIFT, OP_LOWPASS, OP_SPARKFFT, OP_BUCKET, OP_WRITE, OP_MARKS, OP_ROWS, OP_LEVELS, OP_PEAKS, OP_MEANS, OP_POWERS, OP_SPREADS, OP_QUANTILES, OP_BANDS, OP_PICTURE, OP_BURSTS, OP_EMISSIONS, OP_CUTS, OP_SYMBOLS };
struct Op {
    OpKind kind;
    std::string filename; int format = 0; uint64_t sample_rate = 0;     // from
    std::vector<int64_t> cos; double seconds = 1.0;                     // gen
    int64_t shift = 0;                                                  // shift
    uint64_t lp_freq = 0, decimate = 8; size_t size = 40;               // lowpass
    size_t width = 128; uint64_t stride = 128; bool has_range = false; float rmin = 0, rmax = 0;   // sparkfft / bucket
    size_t levels = 2;
    bool has_scan = false; double scan = 0.0;                           // marks -scan SCALE (bits::scan, src/bits.rs)
    bool overwrite = false; std::string prefix;                         // write
    uint64_t pool = 0; bool has_count = false, want_floor = false;      // peaks (-pool P | -count R, count below)
    std::vector<double> qs; std::vector<std::string> q_names;         // quantiles -q 0.5[,0.9,...]
    std::vector<qd_band> bands; bool pick = false, split = false;      // bands (-bins LO:HI[,LO:HI...] | -split K) [-pick]
    uint32_t px_w = 0, px_h = 0, stretch = 4, marker = 0; float scale = 2.29f;   // picture -size PXWxPXH [-stretch 4] [-scan 0] [-scale 2.29]
    bool has_level = false, has_times = false; float level = 0, times = 1; std::string levels_file;   // bursts (-level X | -levels FILE) [-times K]
    uint64_t min_len = 1, cap = 1048576, print_n = 0;                   // bursts [-min 1] [-cap 1048576] [-print 0]
    uint64_t min_cells = 1;                                             // emissions [-cells 1]
    std::string list_file; uint64_t first_window = 0, guard = 1, oversample = 2, cut_taps = 0, cut_pad = 1;   // cuts -list FILE [-first-window 0] [-guard 1] [-oversample 2] [-taps 0] [-pad 1]
    size_t fft = 0; uint64_t step = 0; bool by_level = false;            // symbols -fft w [-step =w] -by freq|level [-range min] [-scan SCALE]
    size_t count = 2048; bool has_slice = false; uint64_t slice_start = 0, slice_end = 0; int windowing = 1;   // rows
    int sink_window = 0;                                                // -window bh|rect of the window-plan verbs (qd_chain_desc.windowing)
};

typedef std::map<std::string, std::vector<std::string>> ArgMap;

// read_just_args (src/args.rs:404-445): "-name value" pairs; a token whose third char is a digit is a number
ArgMap read_just_args(const std::vector<std::string> &argv, size_t &i) {
    ArgMap ret;
    while (i < argv.size()) {
        const std::string &opt = argv[i];
        if (opt.empty() || opt[0] != '-') break;
        if (opt.size() > 2 && isdigit((unsigned char)opt[2])) break;
        ++i;
        if (i >= argv.size()) bail(opt + " requires an argument");
        if (argv[i].empty()) bail(opt + " requires a non-empty argument");
        ret[opt.substr(1)].push_back(argv[i]);
        ++i;
    }
    return ret;
}
std::map<std::string, std::string> no_duplicates(const ArgMap &m) {     // src/args.rs:447-454
    std::map<std::string, std::string> r;
    for (auto &kv : m) {
        if (kv.second.size() != 1) bail("'-" + kv.first + "' specified more than once");
        r[kv.first] = kv.second[0];
    }
    return r;
}
std::string take(std::map<std::string, std::string> &m, const char *k, bool *found) {
    auto it = m.find(k);
    if (it == m.end()) { *found = false; return ""; }
    std::string v = it->second; m.erase(it); *found = true; return v;
}
void ensure_empty(const std::map<std::string, std::string> &m) {
    if (!m.empty()) bail("invalid flags: [\"" + m.begin()->first + "\"]");
}

// guess_details / guess_format_from_name (src/args.rs:65-135,328-333)
void guess_details(const std::string &filename, const std::string *sr_override, const std::string *fmt_override,
                   uint64_t &sample_rate, int &format) {
    std::string sr;
    int fmt = -1;
    std::smatch m;
    if (std::regex_search(filename, m, std::regex("\\bsr([0-9]+[kMG]?)\\b"))) sr = m[1];
    if (std::regex_search(filename, m, std::regex("gqrx_.*?_[0-9]+_([0-9]+)_fc.raw"))) { sr = m[1]; fmt = QD_FMT_CF32; }
    if (std::regex_search(filename, m, std::regex("g\\d+_\\d+(?:\\.\\d+)?M_(\\d+k).cu8"))) { sr = m[1]; fmt = QD_FMT_CU8; }
    size_t dot = filename.rfind('.');
    if (dot != std::string::npos) { int g = format_from_ext(filename.substr(dot + 1)); if (g >= 0) fmt = g; }
    if (sr_override) sr = *sr_override;
    if (fmt_override) { fmt = format_from_ext(*fmt_override); if (fmt < 0) bail("unrecognised extension: \"" + *fmt_override + "\""); }
    if (sr.empty()) bail("unable to guess sample rate from filename \"" + filename + "\", please specify it");
    if (fmt < 0) bail("unable to guess format from filename \"" + filename + "\", please specify it");
    sample_rate = parse_si_u64(sr);
    format = fmt;
}

std::vector<Op> parse(std::vector<std::string> argv) {                 // src/args.rs:19-45
    std::vector<Op> ops;
    size_t i = 0;
    while (i < argv.size()) {
        std::string cmd = argv[i++];
        bool pick = false;
        if (cmd == "bands") {           // -pick is the one flag without a value: it leaves before the "-name value" pairs are read
            for (size_t j = i; j < argv.size() && !argv[j].empty() && argv[j][0] == '-' && !(argv[j].size() > 2 && isdigit((unsigned char)argv[j][2]));) {
                if (argv[j] != "-pick") { j += 2; continue; }
                if (pick) bail("'-pick' specified more than once");
                pick = true;
                argv.erase(argv.begin() + j);
            }
        }
        ArgMap raw = read_just_args(argv, i);
        Op op{};
        // -window bh|rect (default rect) of every verb that builds a window plan through chain_desc: parsed here, once, with `rows -window`'s words
        static const char *const kWindowVerbs[] = {"sparkfft", "bucket", "marks", "levels", "peaks", "means", "powers", "spreads", "quantiles", "bands", "picture", "bursts", "emissions", "symbols"};
        if (std::find_if(std::begin(kWindowVerbs), std::end(kWindowVerbs), [&](const char *v) { return cmd == v; }) != std::end(kWindowVerbs)) {
            auto it = raw.find("window");
            if (it != raw.end()) {
                if (it->second.size() != 1) bail("'-window' specified more than once");
                if (it->second[0] != "bh" && it->second[0] != "rect") bail(cmd + " -window takes bh or rect");
                op.sink_window = it->second[0] == "bh" ? 1 : 0;
                raw.erase(it);
            }
        }
        auto next = [&](const char *err) -> std::string { if (i >= argv.size()) bail(err); return argv[i++]; };
        bool f;
        if (cmd == "from") {
            auto m = no_duplicates(raw);
            std::string fn = next("'from' requires a filename argument");
            std::string sr = take(m, "sr", &f); bool has_sr = f;
            std::string fm = take(m, "format", &f); bool has_fm = f;
            ensure_empty(m);
            op.kind = OP_FROM; op.filename = fn;
            guess_details(fn, has_sr ? &sr : nullptr, has_fm ? &fm : nullptr, op.sample_rate, op.format);
        } else if (cmd == "shift") {
            auto m = no_duplicates(raw);
            if (!m.empty()) bail("'shift' has no named arguments");
            op.kind = OP_SHIFT; op.shift = parse_si_i64(next("'shift' requires a frequency argument"));
        } else if (cmd == "lowpass") {
            auto m = no_duplicates(raw);
            op.kind = OP_LOWPASS;
            op.lp_freq = parse_si_u64(next("'lowpass' requires a frequency argument"));
            std::string v = take(m, "power", &f);
            op.size = f ? (size_t)parse_si_u64(v) * 2 : 40;              // src/args.rs:161-166
            v = take(m, "decimate", &f);
            op.decimate = f ? parse_si_u64(v) : 8;                       // :168-171
            ensure_empty(m);
        } else if (cmd == "sparkfft") {
            auto m = no_duplicates(raw);
            op.kind = OP_SPARKFFT;
            std::string v = take(m, "width", &f);
            op.width = f ? (size_t)parse_si_u64(v) : 128;                // :186-189
            v = take(m, "stride", &f);
            op.stride = f ? parse_si_u64(v) : op.width;                  // :191-194
            v = take(m, "range", &f);
            if (f) {                                                     // :196-207
                size_t c = v.find(':');
                if (c == std::string::npos) bail("range argument must contain a ':': '" + v + "'");
                op.has_range = true;
                op.rmin = strtof(v.substr(0, c).c_str(), nullptr);
                op.rmax = strtof(v.substr(c + 1).c_str(), nullptr);
            }
            ensure_empty(m);
        } else if (cmd == "bucket") {
            auto m = no_duplicates(raw);
            op.kind = OP_BUCKET;
            std::string lv = next("bucket usage: bucket -by freq [number-of-buckets]");
            op.levels = (size_t)strtoull(lv.c_str(), nullptr, 10);
            std::string v = take(m, "width", &f);
            op.width = f ? (size_t)parse_si_u64(v) : 128;
            v = take(m, "stride", &f);
            op.stride = f ? parse_si_u64(v) : op.width;
            v = take(m, "by", &f);
            if (!f || v != "freq") bail("must bucket -by freq");
            ensure_empty(m);
        } else if (cmd == "marks") {
            // not in the reference's grammar: the blank / not-blank byte per sparkfft row that its README derives with sed
            // ("Worked example: OOK in sed"), and optionally bits::scan over it
            auto m = no_duplicates(raw);
            op.kind = OP_MARKS;
            std::string v = take(m, "width", &f);
            op.width = f ? (size_t)parse_si_u64(v) : 128;
            v = take(m, "stride", &f);
            op.stride = f ? parse_si_u64(v) : op.width;
            v = take(m, "min", &f);
            if (f) { op.has_range = true; op.rmin = strtof(v.c_str(), nullptr); op.rmax = 1.0f; }      // (the maximum plays no part)
            v = take(m, "scan", &f);
            if (f) {
                op.has_scan = true; op.scan = strtod(v.c_str(), nullptr);
                if (!std::isfinite(op.scan) || !(op.scan > 0.0)) bail("marks -scan takes a scale > 0");
            }
            ensure_empty(m);
        } else if (cmd == "levels") {
            // not in the reference's grammar: the level summary of the windows sparkfft would print (FftResult::max / min, src/ffts.rs:101-107,
            // and the `min max` line of src/ui/mod.rs:317-409): what -range to pass and where in the band the signal sits
            auto m = no_duplicates(raw);
            op.kind = OP_LEVELS;
            std::string v = take(m, "width", &f);
            op.width = f ? (size_t)parse_si_u64(v) : 128;
            v = take(m, "stride", &f);
            op.stride = f ? parse_si_u64(v) : op.width;
            ensure_empty(m);
        } else if (cmd == "peaks" || cmd == "means" || cmd == "powers" || cmd == "spreads") {
            // not in the reference's grammar: the spectrum analyser's max-hold picture — every window sparkfft would print, each group of
            // `pool` consecutive windows folded per bin into one row (qd_plan_pool) — its average trace (qd_plan_mean), its RMS trace (qd_plan_power) and its deviation trace (qd_plan_spread)
            auto m = no_duplicates(raw);
            op.kind = cmd == "peaks" ? OP_PEAKS : cmd == "means" ? OP_MEANS : cmd == "powers" ? OP_POWERS : OP_SPREADS;
            std::string v = take(m, "width", &f);
            op.width = f ? (size_t)parse_si_u64(v) : 128;
            v = take(m, "stride", &f);
            op.stride = f ? parse_si_u64(v) : op.width;
            v = take(m, "pool", &f);
            if (f) { op.pool = parse_si_u64(v); if (!op.pool) bail(cmd + " -pool takes a number of windows > 0"); }
            v = take(m, "count", &f);
            op.has_count = f;
            op.count = f ? (size_t)parse_si_u64(v) : 2048;
            if (op.has_count && op.pool) bail(cmd + " takes -pool or -count, not both");
            if (!op.count) bail(cmd + " -count takes a number of rows > 0");
            v = take(m, "range", &f);
            if (f) {
                size_t c = v.find(':');
                if (c == std::string::npos) bail("range argument must contain a ':': '" + v + "'");
                op.has_range = true;
                op.rmin = strtof(v.substr(0, c).c_str(), nullptr);
                op.rmax = strtof(v.substr(c + 1).c_str(), nullptr);
            }
            if (op.kind == OP_PEAKS) {
                v = take(m, "floor", &f);
                op.want_floor = f ? parse_bool(v) : false;
            }
            ensure_empty(m);
            op.prefix = next(("'" + cmd + "' requires a prefix argument").c_str());
        } else if (cmd == "quantiles") {
            // not in the reference's grammar: the percentile traces of the windows sparkfft would print — per bin of each group of `pool`
            // consecutive windows the level that holds the group's q-quantile (qd_plan_density), one picture per q
            auto m = no_duplicates(raw);
            op.kind = OP_QUANTILES;
            std::string v = take(m, "width", &f);
            op.width = f ? (size_t)parse_si_u64(v) : 128;
            v = take(m, "stride", &f);
            op.stride = f ? parse_si_u64(v) : op.width;
            v = take(m, "pool", &f);
            if (f) { op.pool = parse_si_u64(v); if (!op.pool) bail("quantiles -pool takes a number of windows > 0"); }
            v = take(m, "count", &f);
            op.has_count = f;
            op.count = f ? (size_t)parse_si_u64(v) : 2048;
            if (op.has_count && op.pool) bail("quantiles takes -pool or -count, not both");
            if (!op.count) bail("quantiles -count takes a number of rows > 0");
            v = take(m, "q", &f);
            if (!f) bail("quantiles requires -q");
            for (size_t a = 0; a <= v.size();) {
                size_t c = v.find(',', a);
                if (c == std::string::npos) c = v.size();
                const std::string tok = v.substr(a, c - a);
                char *end = nullptr;
                const double q = strtod(tok.c_str(), &end);
                if (tok.empty() || *end || !(q >= 0.0 && q <= 1.0)) bail("quantiles -q takes numbers in [0, 1] separated by commas: '" + v + "'");
                op.qs.push_back(q); op.q_names.push_back(tok);
                a = c + 1;
            }
            if (op.qs.size() > 8) bail("quantiles -q takes at most 8 quantiles");
            v = take(m, "range", &f);
            if (!f) bail("quantiles requires -range");
            {
                size_t c = v.find(':');
                if (c == std::string::npos) bail("range argument must contain a ':': '" + v + "'");
                op.has_range = true;
                op.rmin = strtof(v.substr(0, c).c_str(), nullptr);
                op.rmax = strtof(v.substr(c + 1).c_str(), nullptr);
            }
            ensure_empty(m);
            op.prefix = next("'quantiles' requires a prefix argument");
        } else if (cmd == "bands") {
            // not in the reference's grammar: the band traces of the windows sparkfft would print — per window and band of fftshifted bins
            // the level, and the bin of the peak (qd_plan_bands); with -pick the loudest band per window as one line of digits, what
            // `bucket -by freq K` would print
            auto m = no_duplicates(raw);
            op.kind = OP_BANDS; op.pick = pick;
            std::string v = take(m, "width", &f);
            op.width = f ? (size_t)parse_si_u64(v) : 128;
            v = take(m, "stride", &f);
            op.stride = f ? parse_si_u64(v) : op.width;
            v = take(m, "bins", &f);
            const bool has_bins = f;
            if (f) {
                for (size_t a = 0; a <= v.size();) {
                    size_t c = v.find(',', a);
                    if (c == std::string::npos) c = v.size();
                    const std::string tok = v.substr(a, c - a);
                    const size_t colon = tok.find(':');
                    char *e0 = nullptr, *e1 = nullptr;
                    const std::string los = tok.substr(0, colon), his = colon == std::string::npos ? "" : tok.substr(colon + 1);
                    const unsigned long long lo = strtoull(los.c_str(), &e0, 10), hi = strtoull(his.c_str(), &e1, 10);
                    if (los.empty() || his.empty() || !isdigit((unsigned char)los[0]) || !isdigit((unsigned char)his[0]) || *e0 || *e1 || lo >= hi || hi > op.width)
                        bail("bands -bins takes LO:HI[,LO:HI...] with 0 <= LO < HI <= width: '" + v + "'");
                    op.bands.push_back(qd_band{(uint32_t)lo, (uint32_t)hi});
                    a = c + 1;
                }
            }
            v = take(m, "split", &f);
            if (f && has_bins) bail("bands takes -bins or -split, not both");
            if (!f && !has_bins) bail("bands requires -bins or -split");
            if (f) {
                const uint64_t K = parse_si_u64(v);
                if (!K || op.width % K) bail("bands -split takes a number of bands > 0 that divides the width");
                op.split = true;
                if (K <= QD_BANDS_MAX)
                    for (uint64_t k = 0; k < K; ++k) op.bands.push_back(qd_band{(uint32_t)(k * (op.width / K)), (uint32_t)((k + 1) * (op.width / K))});
                else op.bands.resize(K);
            }
            if (op.bands.size() > QD_BANDS_MAX) bail("bands takes at most " + std::to_string(QD_BANDS_MAX) + " bands");
            if (op.pick && op.bands.size() > 36) bail("bands -pick prints one digit a window: at most 36 bands");
            ensure_empty(m);
            op.prefix = next("'bands' requires a prefix argument");
        } else if (cmd == "bursts" || cmd == "emissions") {
            // not in the reference's grammar: a threshold per fftshifted bin applied to the windows sparkfft would print, and the list of
            // on/off runs per bin (qd_plan_bursts), or of the connected regions of on cells (qd_plan_emissions): what happened when
            const bool em = cmd == "emissions";
            auto m = no_duplicates(raw);
            op.kind = em ? OP_EMISSIONS : OP_BURSTS;
            std::string v = take(m, "width", &f);
            op.width = f ? (size_t)parse_si_u64(v) : 128;
            v = take(m, "stride", &f);
            op.stride = f ? parse_si_u64(v) : op.width;
            auto number = [&](const std::string &t, const char *flag) {
                char *e = nullptr;
                const float x = strtof(t.c_str(), &e);
                if (t.empty() || *e) bail(cmd + " " + flag + " takes a number: '" + t + "'");
                return x;
            };
            v = take(m, "level", &f);
            op.has_level = f;
            if (f) op.level = number(v, "-level");
            v = take(m, "levels", &f);
            if (f && op.has_level) bail(cmd + " takes -level or -levels, not both");
            if (!f && !op.has_level) bail(cmd + " requires -level or -levels");
            if (f) op.levels_file = v;
            v = take(m, "times", &f);
            op.has_times = f;
            if (f) op.times = number(v, "-times");
            v = take(m, "min", &f);
            if (f) { op.min_len = parse_si_u64(v); if (!op.min_len) bail(cmd + " -min takes a number of windows > 0"); }
            v = take(m, "cap", &f);
            if (f) {
                op.cap = parse_si_u64(v);
                if (!em && op.cap > QD_BURSTS_MAX_WORKSPACE / sizeof(qd_burst)) bail("bursts -cap takes at most 33554432 records");
                if (em && op.cap > QD_EMISSIONS_MAX_WORKSPACE / sizeof(qd_emission)) bail("emissions -cap takes at most 19173961 records");
            }
            if (em) {
                v = take(m, "cells", &f);
                if (f) { op.min_cells = parse_si_u64(v); if (!op.min_cells) bail("emissions -cells takes a number of cells > 0"); }
            }
            v = take(m, "print", &f);
            if (f) op.print_n = parse_si_u64(v);
            ensure_empty(m);
            op.prefix = next(em ? "'emissions' requires a prefix argument" : "'bursts' requires a prefix argument");
        } else if (cmd == "cuts" || cmd == "symbols") {
            // not in the reference's grammar: the IQ of every record of an `emissions` list, cut out of the source in one call (qd_cuts_run) -
            // and, as `symbols`, the digits (`bucket -by freq 2`) or blank / non-blank rows (sparkfft) of every cut, the IQ staying on the
            // device (qd_cuts_symbols).  The chain words in front describe the plan the list came from, -width and -stride its windows
            auto m = no_duplicates(raw);
            const bool sym = cmd == "symbols";
            op.kind = sym ? OP_SYMBOLS : OP_CUTS;
            std::string v = take(m, "width", &f);
            if (!f) bail(cmd + " requires -width, the width of the plan the list came from");
            op.width = (size_t)parse_si_u64(v);
            v = take(m, "stride", &f);
            op.stride = f ? parse_si_u64(v) : op.width;
            v = take(m, "list", &f);
            if (!f) bail(cmd + " requires -list FILE.emissions");
            op.list_file = v;
            auto u32 = [&](const char *flag, uint64_t deflt, uint64_t least) {
                const std::string t = take(m, flag, &f);
                if (!f) return deflt;
                const uint64_t k = parse_si_u64(t);
                if (k < least || k > 0xffffffffull) bail(cmd + " -" + flag + " takes a number from " + std::to_string(least) + " to 4294967295");
                return k;
            };
            v = take(m, "first-window", &f);
            if (f) op.first_window = parse_si_u64(v);
            op.guard = u32("guard", 1, 0);
            op.oversample = u32("oversample", 2, 1);
            op.cut_pad = u32("pad", 1, 0);
            v = take(m, "taps", &f);
            if (f) { op.cut_taps = parse_si_u64(v); if (op.cut_taps == 1 || op.cut_taps > QD_CUT_MAX_TAPS) bail(cmd + " -taps takes 0 (from the decimation) or 2 ... 4096"); }
            v = take(m, "print", &f);
            if (f) op.print_n = parse_si_u64(v);
            if (sym) {
                v = take(m, "fft", &f);
                if (!f) bail("symbols requires -fft, the width of the windows over each cut");
                op.fft = (size_t)parse_si_u64(v);
                v = take(m, "step", &f);
                op.step = f ? parse_si_u64(v) : op.fft;
                v = take(m, "by", &f);
                if (!f || (v != "freq" && v != "level")) bail("symbols -by takes freq (the bucket sink's digits) or level (the mark sink's blank / non-blank rows)");
                op.by_level = v == "level";
                v = take(m, "range", &f);
                if (f) {
                    if (!op.by_level) bail("symbols -range is the mark sink's minimum: it goes with -by level");
                    op.has_range = true; op.rmin = strtof(v.c_str(), nullptr); op.rmax = 1.0f;
                }
                v = take(m, "scan", &f);
                if (f) {
                    op.has_scan = true; op.scan = strtod(v.c_str(), nullptr);
                    if (!std::isfinite(op.scan) || !(op.scan > 0.0)) bail("symbols -scan takes a scale > 0");
                }
            }
            ensure_empty(m);
            op.prefix = next(sym ? "'symbols' requires a prefix argument" : "'cuts' requires a prefix argument");
        } else if (cmd == "picture") {
            // not in the reference's grammar: the waterfall its conrod front end renders (src/ui/mod.rs:294-412) as a binary PPM.  -width 8,
            // -stride 1 and -stretch 4 are its Params (:72-76) and 2.29 its scale (:353); -scan 0, no marker columns, is not: its default of 1
            // blackens every column
            auto m = no_duplicates(raw);
            op.kind = OP_PICTURE;
            std::string v = take(m, "width", &f);
            op.width = f ? (size_t)parse_si_u64(v) : 8;
            v = take(m, "stride", &f);
            op.stride = f ? parse_si_u64(v) : 1;
            v = take(m, "size", &f);
            if (!f) bail("picture requires -size PXWxPXH");
            {
                const size_t x = v.find('x');
                char *e0 = nullptr, *e1 = nullptr;
                const std::string ws = v.substr(0, x), hs = x == std::string::npos ? "" : v.substr(x + 1);
                const unsigned long long pw = strtoull(ws.c_str(), &e0, 10), ph = strtoull(hs.c_str(), &e1, 10);
                if (ws.empty() || hs.empty() || !isdigit((unsigned char)ws[0]) || !isdigit((unsigned char)hs[0]) || *e0 || *e1 || !pw || !ph || pw > 0xffffffffull || ph > 0xffffffffull)
                    bail("picture -size takes PXWxPXH, both > 0: '" + v + "'");
                op.px_w = (uint32_t)pw; op.px_h = (uint32_t)ph;
            }
            v = take(m, "stretch", &f);
            if (f) { const uint64_t k = parse_si_u64(v); if (!k || k > 0xffffffffull) bail("picture -stretch takes a number of pixel rows > 0"); op.stretch = (uint32_t)k; }
            v = take(m, "scan", &f);
            if (f) { const uint64_t k = parse_si_u64(v); if (k > 0xffffffffull) bail("picture -scan takes 0 or a number of windows"); op.marker = (uint32_t)k; }
            v = take(m, "scale", &f);
            if (f) { char *e = nullptr; op.scale = strtof(v.c_str(), &e); if (*e || !(op.scale > 0.f) || std::isinf(op.scale)) bail("picture -scale takes a finite number > 0: '" + v + "'"); }
            v = take(m, "overwrite", &f);
            op.overwrite = f ? parse_bool(v) : false;
            ensure_empty(m);
            op.prefix = next("'picture' requires a prefix argument");
        } else if (cmd == "rows") {
            // not in the reference's grammar: the rows of its spectrogram view (take_fft, src/ffts.rs:18-85) as a greyscale picture
            auto m = no_duplicates(raw);
            op.kind = OP_ROWS;
            std::string v = take(m, "width", &f);
            op.width = f ? (size_t)parse_si_u64(v) : 512;                // src/eui/mod.rs:66
            v = take(m, "count", &f);
            op.count = f ? (size_t)parse_si_u64(v) : 2048;               // :87
            v = take(m, "slice", &f);
            if (f) {
                size_t c = v.find(':');
                if (c == std::string::npos) bail("slice argument must contain a ':': '" + v + "'");
                op.has_slice = true;
                op.slice_start = parse_si_u64(v.substr(0, c));
                op.slice_end = parse_si_u64(v.substr(c + 1));
            }
            v = take(m, "window", &f);
            if (f && v != "bh" && v != "rect") bail("rows -window takes bh or rect");
            op.windowing = (f && v == "rect") ? 0 : 1;
            ensure_empty(m);
            op.prefix = next("'rows' requires a prefix argument");
        } else if (cmd == "write") {
            auto m = no_duplicates(raw);
            op.kind = OP_WRITE;
            std::string v = take(m, "overwrite", &f);
            op.overwrite = f ? parse_bool(v) : false;
            ensure_empty(m);
            op.prefix = next("'write' requires a prefix argument");
        } else if (cmd == "gen") {
            op.kind = OP_GEN;
            auto it = raw.find("cos");
            if (it == raw.end()) bail("gen requires at least one operation");
            for (auto &s : it->second) op.cos.push_back(parse_si_i64(s));
            raw.erase(it);
            auto il = raw.find("len");
            if (il != raw.end()) {
                if (il->second.size() != 1) bail("len requires exactly one value");
                op.seconds = parse_si_f64(il->second[0]);
                raw.erase(il);
            }
            if (!raw.empty()) bail("invalid flags: [\"" + raw.begin()->first + "\"]");
            op.sample_rate = parse_si_u64(next("sample rate argument required"));
        } else if (cmd == "ui" || cmd == "eui") {
            bail("'" + cmd + "' (GUI) is out of scope of the MI355X engine");
        } else {
            bail("processing command: \"" + cmd + "\": unrecognised command");
        }
        ops.push_back(op);
    }
    return ops;
}

// ------------------------------------------------------------------ Samples iterator (src/samples.rs:11-28)

const size_t PANIC = (size_t)-1;

struct Samples {
    virtual ~Samples() {}
    virtual uint64_t len() const = 0;
    virtual uint64_t sample_rate() const = 0;
    virtual size_t read_at(uint64_t off, qd_c32 *buf, size_t n) const = 0;
    void read_exact_at(uint64_t off, qd_c32 *buf, size_t n) const {
        size_t got = read_at(off, buf, n);
        if (got != n) bail("TODO: read-exact messed up: " + std::to_string(n) + " (wanted) != " + std::to_string(got) +
                           " (read) at " + std::to_string(off));
    }
};

struct SampleFile : Samples {                                           // src/samples.rs:44-94
    int fd, format; uint64_t file_len, rate;
    SampleFile(const std::string &fn, int fmt, uint64_t sr) : format(fmt), rate(sr) {
        fd = open(fn.c_str(), O_RDONLY);
        if (fd < 0) bail(std::string(strerror(errno)) + " (os error " + std::to_string(errno) + ")");
        struct stat st; fstat(fd, &st); file_len = (uint64_t)st.st_size;
    }
    ~SampleFile() override { if (fd >= 0) close(fd); }
    uint64_t len() const override { return file_len / qd_pair_bytes(format); }
    uint64_t sample_rate() const override { return rate; }
    size_t read_at(uint64_t off, qd_c32 *into, size_t n) const override {
        if (!(off < len())) bail("assertion failed: off < self.len()");  // :74
        const uint64_t pb = qd_pair_bytes(format);
        std::vector<uint8_t> buf(pb * n);
        ssize_t got = pread(fd, buf.data(), buf.size(), (off_t)(off * pb));
        if (got < 0) bail("read");
        size_t bytes = (size_t)got - (size_t)got % pb;                   // :84
        size_t pairs = bytes / pb;
        if (pairs) qd_check(qd_unpack(format, buf.data(), pairs, into, QD_MEM_HOST), "unpack");
        return pairs;
    }
};

struct Gen : Samples {                                                  // src/gen.rs:16-52
    std::vector<int64_t> cos; uint64_t rate; double seconds;
    Gen(std::vector<int64_t> c, uint64_t sr, double s) : cos(std::move(c)), rate(sr), seconds(s) {
        if (cos.empty()) bail("cos cannot be empty");
        if (rate == 0) bail("sample rate may not be zero");
        if (!(seconds > 0.0)) bail("seconds may not be <= 0");
    }
    uint64_t len() const override {
        double v = seconds * (double)rate;
        return !(v > 0) ? 0 : (v >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)v);
    }
    uint64_t sample_rate() const override { return rate; }
    size_t read_at(uint64_t off, qd_c32 *buf, size_t n) const override {
        if (n) qd_check(qd_gen(cos.data(), cos.size(), rate, off, n, buf, QD_MEM_HOST), "gen");
        return n;
    }
};

struct Shift : Samples {                                                // src/shift.rs
    std::unique_ptr<Samples> inner; double ratio; uint64_t rate;
    Shift(std::unique_ptr<Samples> in, int64_t freq) : inner(std::move(in)) {
        rate = inner->sample_rate();
        int64_t af = freq < 0 ? -freq : freq;
        if (!(af < (int64_t)(rate / 2))) bail("frequency must be under half the sample rate");
        ratio = qd_shift_ratio(freq, rate);
    }
    uint64_t len() const override { return inner->len(); }
    uint64_t sample_rate() const override { return rate; }
    size_t read_at(uint64_t off, qd_c32 *buf, size_t n) const override {
        size_t valid = inner->read_at(off, buf, n);
        if (valid) qd_check(qd_shift(buf, valid, off, ratio, QD_MEM_HOST), "shift");
        return valid;
    }
};

struct LowPass : Samples {                                              // src/filter.rs
    std::unique_ptr<Samples> inner; std::vector<float> taps; uint64_t decimate, orig_rate;
    LowPass(std::unique_ptr<Samples> in, uint64_t freq, uint64_t dec, size_t size) : inner(std::move(in)), taps(size), decimate(dec) {
        orig_rate = inner->sample_rate();
        qd_check(qd_lowpass_design(freq, orig_rate, size, taps.data()), "lowpass_design");
    }
    uint64_t len() const override {
        if (inner->len() < taps.size()) bail("assertion failed: self.inner.len() >= self.filter.len()");
        return 1 + (inner->len() - taps.size()) / decimate;
    }
    uint64_t sample_rate() const override { return orig_rate / decimate; }
    size_t read_at(uint64_t off, qd_c32 *buf, size_t n) const override {
        std::vector<qd_c32> raw(n * decimate + taps.size());             // :68-69
        size_t valid = inner->read_at(off * decimate, raw.data(), raw.size());
        size_t produced = 0;
        qd_check(qd_lowpass_block(taps.data(), taps.size(), decimate, raw.data(), valid, buf, n, &produced, QD_MEM_HOST), "lowpass");
        return produced;
    }
};

// ------------------------------------------------------------------ sinks

struct ChainSpec {          // what a fused plan can express
    bool fusable = false;
    const Op *src = nullptr, *shift = nullptr, *lowpass = nullptr;
    std::vector<const Op *> stages;      // every shift / lowpass since the source, in order (cascade plans)
    bool cascade = false;                // the stages are not  [shift] [lowpass]: qd_plan_create_stages
};

// The whole source file for a fused plan: mapped, not read — and registered with the HIP runtime when it allows it, so the
// engine copies straight out of the page cache (QD_MEM_HOST_PINNED) instead of staging every chunk through a pinned ring.
struct MappedFile {
    const uint8_t *p = nullptr;
    size_t size = 0;
    int mem = QD_MEM_HOST;
    explicit MappedFile(const std::string &fn) {
        int fd = open(fn.c_str(), O_RDONLY);
        if (fd < 0) bail(std::string(strerror(errno)) + ": " + fn);
        struct stat st;
        if (fstat(fd, &st) != 0) { close(fd); bail(std::string(strerror(errno)) + ": " + fn); }
        size = (size_t)st.st_size;
        if (size) {
            void *m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) { close(fd); bail(std::string(strerror(errno)) + ": " + fn); }
            p = static_cast<const uint8_t *>(m);
            if (size >= (64u << 20) && qd_host_register(m, size) == QD_OK) mem = QD_MEM_HOST_PINNED;   // small files: not worth pinning
        }
        close(fd);
    }
    ~MappedFile() {
        if (p) {
            if (mem == QD_MEM_HOST_PINNED) (void)qd_host_unregister(const_cast<uint8_t *>(p));
            munmap(const_cast<uint8_t *>(p), size);
        }
    }
    MappedFile(const MappedFile &) = delete;
    MappedFile &operator=(const MappedFile &) = delete;
};

int g_gpus = 1;      // `-gpus N` in front of the chain: shard the sink's windows over N devices (qd_plan_run_sharded)

// plan for the CLI: the library's defaults, plus window-range shards over g_gpus devices (repeating devices when the
// machine has fewer: the shards then run as independent streams of one device)
// (`stages` of a cascade, empty for a one-stage plan; gpus = 1: an unsharded plan on the current device)
int create_plan(const qd_chain_desc &d, qd_plan **plan, const std::vector<qd_stage> &stages, int gpus = g_gpus) {
    const bool casc = !stages.empty();
    if (gpus <= 1) return casc ? qd_plan_create_stages(&d, stages.data(), stages.size(), nullptr, plan) : qd_plan_create(&d, plan);
    qd_plan_options o{};
    o.struct_size = sizeof o;
    int n_dev = 1;
    if (qd_device_count(&n_dev) != QD_OK || n_dev < 1) n_dev = 1;
    o.n_shards = (uint32_t)(gpus > QD_MAX_SHARDS ? QD_MAX_SHARDS : gpus);
    for (uint32_t g = 0; g < o.n_shards; ++g) o.shard_device[g] = (int32_t)(g % (uint32_t)n_dev);
    return casc ? qd_plan_create_stages(&d, stages.data(), stages.size(), &o, plan) : qd_plan_create_ex(&d, &o, plan);
}

// device buffer that frees itself (the `gen` source of a fused chain lives in HBM)
struct DeviceBuf {
    void *p = nullptr;
    ~DeviceBuf() { if (p) qd_device_free(p); }
};

// the first n samples of a `gen` source, produced on the device (src/gen.rs:30-47): they never cross PCIe
void gen_to_device(const Op &src, uint64_t n, DeviceBuf *buf) {
    qd_check(qd_device_alloc((size_t)n * 8, &buf->p), "device buffer for gen");
    const uint64_t piece = 1ull << 28;                                   // Gen::read_at in pieces: bounded kernel launches
    for (uint64_t a = 0; a < n; a += piece)
        qd_check(qd_gen(src.cos.data(), src.cos.size(), src.sample_rate, a, (size_t)std::min(n - a, piece), static_cast<qd_c32 *>(buf->p) + a, QD_MEM_DEVICE), "gen");
}

// The source of a fused plan: the whole file, mapped, or a `gen` stream, which resident() produces on the device when first asked for.
struct ChainSource {
    const Op &op;
    const bool from_gen;
    std::unique_ptr<MappedFile> data;
    DeviceBuf gen;
    uint64_t n_samples;
    explicit ChainSource(const ChainSpec &cs) : op(*cs.src), from_gen(op.kind == OP_GEN) {
        if (!from_gen) data.reset(new MappedFile(op.filename));
        n_samples = from_gen ? (uint64_t)(op.seconds * (double)op.sample_rate)                  // Gen::len, src/gen.rs:32
                             : data->size / qd_pair_bytes(op.format);
    }
    const void *resident(int *mem) {
        if (!from_gen) { *mem = data->mem; return data->p; }
        if (!gen.p) gen_to_device(op, n_samples, &gen);
        *mem = QD_MEM_DEVICE;
        return gen.p;
    }
};

// what a fused plan is made from: the source, the chain's [shift] [lowpass] (or, for a cascade, its stages) and the sink's windows
void chain_desc(const ChainSpec &cs, const ChainSource &in, size_t width, uint64_t stride, int epilogue, qd_chain_desc *d, std::vector<qd_stage> *stages, int windowing = 0) {
    *d = qd_chain_desc{};
    d->struct_size = sizeof *d;
    d->format = in.from_gen ? QD_FMT_CF32 : cs.src->format; d->sample_rate = cs.src->sample_rate;
    d->n_samples = in.n_samples;
    stages->clear();
    if (cs.cascade) {
        for (const Op *op : cs.stages) {
            qd_stage st{};
            if (op->kind == OP_SHIFT) { st.kind = QD_STAGE_SHIFT; st.shift_hz = op->shift; }
            else { st.kind = QD_STAGE_LOWPASS; st.lowpass_hz = op->lp_freq; st.decimate = op->decimate; st.taps = op->size; }
            stages->push_back(st);
        }
    } else {
        if (cs.shift) { d->has_shift = 1; d->shift_hz = cs.shift->shift; }
        if (cs.lowpass) { d->has_lowpass = 1; d->lowpass_hz = cs.lowpass->lp_freq; d->decimate = cs.lowpass->decimate; d->taps = cs.lowpass->size; }
    }
    d->width = width; d->stride = stride; d->epilogue = epilogue;
    d->windowing = windowing;
}

int sink_epilogue(const Op &sink) {
    return sink.kind == OP_BUCKET ? QD_EPI_BUCKET2_U8 : (sink.kind == OP_MARKS ? QD_EPI_MARK_U8 : QD_EPI_GLYPH_U8);
}

// the `marks` sink's output: one line of 0 / 1 digits, or with -scan the bits of bits::scan over them and its error on a second line
void print_marks(const uint8_t *marks, uint64_t n, const Op &sink) {
    if (!sink.has_scan) {
        std::string digits;
        for (uint64_t w = 0; w < n; ++w) digits.push_back((char)('0' + (marks[w] ? 1 : 0)));
        printf("%s\n", digits.c_str());
        return;
    }
    std::vector<uint8_t> bits((size_t)n + 1);
    size_t produced = 0;
    double error = 0.0;
    int rc = qd_bits_scan(marks, (size_t)n, sink.scan, bits.data(), bits.size(), &produced, &error);
    if (rc == QD_ERR_INVALID && produced > bits.size()) {                // (a scale below 1 emits more bits than marks)
        bits.resize(produced);
        rc = qd_bits_scan(marks, (size_t)n, sink.scan, bits.data(), bits.size(), &produced, &error);
    }
    qd_check(rc, "scan");                                                // the non-terminating case: the library's message, exit 1
    std::string digits;
    for (size_t b = 0; b < produced; ++b) digits.push_back((char)('0' + bits[b]));
    printf("%s\n%.17g\n", digits.c_str(), error);
}

// sparkfft / bucket through ONE fused plan over the whole file — or over a `gen` stream that is produced on the device
// (src/gen.rs:30-47) and never crosses PCIe: only the glyph codes / digits come back
// returns false when the library has no fused plan for the chain (QD_ERR_UNSUPPORTED: e.g. overlapping windows whose FIR input exceeds one
// workgroup's LDS); the header line is printed by then, the caller pulls the windows through the iterator chain instead
// A cascade whose last window(s) fail read_exact_at (two lowpasses: LowPass::len over-reports, src/filter.rs:45-48): the complete
// windows' rows are printed, then the first failing window is read through the iterator chain, which stops with the reference's
// error (src/samples.rs:17-27) — sparkfft prints inside its loop (src/fft.rs:28-65), bucket unwraps before printing anything.
bool run_fused(const ChainSpec &cs, const Op &sink, const Samples &samples) {
    const uint64_t out_rate = samples.sample_rate();
    ChainSource in(cs);
    const bool from_gen = in.from_gen;
    qd_chain_desc d;
    std::vector<qd_stage> stages;
    chain_desc(cs, in, sink.width, sink.stride, sink_epilogue(sink), &d, &stages, sink.sink_window);
    d.has_range = sink.has_range; d.range_min = sink.rmin; d.range_max = sink.rmax;
    if (sink.kind == OP_SPARKFFT) printf("sparkfft sample_rate=%" PRIu64 "\n", out_rate);   // printed before any read (src/fft.rs:19)
    qd_plan *plan = nullptr;
    {
        const int rc = create_plan(d, &plan, stages, from_gen ? 1 : g_gpus);
        if (rc == QD_ERR_UNSUPPORTED) return false;
        qd_check(rc, "plan");
    }
    qd_plan_info info;
    qd_check(qd_plan_get_info(plan, &info), "plan info");
    uint64_t complete = info.n_windows;
    qd_check(qd_plan_complete_windows(plan, &complete), "plan complete windows");
    // a range past the complete windows returns QD_ERR_SHORT after writing every complete window
    auto check_run = [&](int rc, const char *what) { if (!(rc == QD_ERR_SHORT && complete < info.n_windows)) qd_check(rc, what); };
    std::vector<uint8_t> out(info.n_windows * info.out_bytes_per_window + 1);
    if (info.n_windows && !from_gen) {
        if (g_gpus > 1) check_run(qd_plan_run_sharded(plan, in.data->p, in.data->mem, out.data(), QD_MEM_HOST), "run (sharded)");
        else check_run(qd_plan_run(plan, in.data->p, in.data->mem, 0, d.n_samples, 0, info.n_windows, out.data(), QD_MEM_HOST, nullptr), "run");
    }
    if (info.n_windows && from_gen) {
        DeviceBuf dst;
        const size_t ob = (size_t)(info.n_windows * info.out_bytes_per_window);
        int mem = QD_MEM_DEVICE;
        const void *src = in.resident(&mem);
        qd_check(qd_device_alloc(ob, &dst.p), "device buffer for the sink");
        check_run(qd_plan_run(plan, src, mem, 0, d.n_samples, 0, info.n_windows, dst.p, QD_MEM_DEVICE, nullptr), "run");
        qd_check(qd_device_copy(out.data(), QD_MEM_HOST, dst.p, QD_MEM_DEVICE, ob), "copy back");   // synchronises with the launch
    }
    qd_plan_destroy(plan);
    if (sink.kind == OP_SPARKFFT) {
        // header already printed; rows only
        std::string line;
        for (uint64_t w = 0; w < complete; ++w) {
            line.assign("\xE2\x94\x82");
            for (size_t b = 0; b < sink.width; ++b) {
                uint8_t c = out[w * sink.width + b];
                if (c == 0) line.push_back(' ');
                else if (c <= 8) { line.push_back((char)0xE2); line.push_back((char)0x96); line.push_back((char)(0x80 + c)); }
                else bail("index out of bounds: the len is 7 but the index is 7");
            }
            line += "\xE2\x94\x82\n";
            fwrite(line.data(), 1, line.size(), stdout);
        }
    }
    if (complete < info.n_windows) {
        std::vector<qd_c32> buf(sink.width);
        samples.read_exact_at(complete * sink.stride, buf.data(), sink.width);       // fails: the reference's error
        bail("complete-window count disagrees with the iterator chain");
    }
    if (sink.kind == OP_MARKS) print_marks(out.data(), info.n_windows, sink);
    else if (sink.kind != OP_SPARKFFT) {
        std::string digits;
        for (uint64_t w = 0; w < info.n_windows; ++w) digits.push_back((char)('0' + out[w]));
        printf("%s\n", digits.c_str());                                   // src/lib.rs:144-158
    }
    return true;
}

// -window on the iterator path: sample k of each gathered window times qd_window_design's w[k], as Complex<f32> * f32 — the two separately
// rounded products the fused plans form (a product alone has nothing to contract with; the build passes -ffp-contract=off all the same)
void window_gathered(qd_c32 *buf, uint64_t nb, size_t W, const Op &sink) {
    if (!sink.sink_window) return;
    std::vector<float> w(W);
    qd_check(qd_window_design(sink.sink_window, W, w.data()), "window");
    for (uint64_t i = 0; i < nb; ++i)
        for (size_t k = 0; k < W; ++k) { qd_c32 &v = buf[i * W + k]; v.re = v.re * w[k]; v.im = v.im * w[k]; }
}

// FFT + epilogue of nb gathered windows (contiguous, stride W) on the GPU: a no-shift/no-lowpass plan
std::vector<uint8_t> sink_batch(const qd_c32 *buf, uint64_t nb, size_t W, const Op &sink) {
    qd_chain_desc d{};
    d.struct_size = sizeof d;
    d.format = QD_FMT_CF32; d.sample_rate = 1;
    // len such that the sink's own loop yields exactly nb windows at stride W
    d.n_samples = sink.kind == OP_BUCKET ? (nb + 1) * W : nb * W + 1;
    d.width = W; d.stride = W;
    d.epilogue = sink_epilogue(sink);
    d.has_range = sink.has_range; d.range_min = sink.rmin; d.range_max = sink.rmax;
    qd_plan *plan = nullptr;
    qd_check(qd_plan_create(&d, &plan), "plan");
    qd_plan_info info;
    qd_check(qd_plan_get_info(plan, &info), "plan info");
    std::vector<uint8_t> out(nb * info.out_bytes_per_window + 1);
    int rc = qd_plan_run(plan, buf, QD_MEM_HOST, 0, nb * W, 0, nb, out.data(), QD_MEM_HOST, nullptr);
    qd_plan_destroy(plan);
    qd_check(rc, "run");
    return out;
}

// the same sinks over an arbitrary iterator chain: windows are pulled through read_exact_at exactly as
// the reference does (src/fft.rs:30,91), gathered, and transformed in batches on the GPU
void run_iter_sink(const Samples &s, const Op &sink, bool header_printed = false) {
    const size_t W = sink.width; const uint64_t S = sink.stride;
    if (sink.kind == OP_SPARKFFT && !header_printed) printf("sparkfft sample_rate=%" PRIu64 "\n", s.sample_rate());
    if (!W || (W & (W - 1))) bail("Radix4 algorithm requires a power-of-two input size");
    if (S == 0) bail("stride 0 never terminates");
    uint64_t len = s.len();
    if (len < W) bail("attempt to subtract with overflow");               // src/fft.rs:28 / :86
    uint64_t lim = len - W;
    uint64_t nwin = sink.kind == OP_BUCKET ? lim / S : (lim == 0 ? 0 : (lim - 1) / S + 1);
    const uint64_t batch = 4096;
    std::vector<qd_c32> buf(batch * W);
    std::string digits;
    std::vector<uint8_t> marks;
    for (uint64_t w0 = 0; w0 < nwin; w0 += batch) {
        uint64_t nb = nwin - w0 < batch ? nwin - w0 : batch;
        for (uint64_t i = 0; i < nb; ++i) s.read_exact_at((w0 + i) * S, buf.data() + i * W, W);
        window_gathered(buf.data(), nb, W, sink);
        std::vector<uint8_t> out = sink_batch(buf.data(), nb, W, sink);
        if (sink.kind == OP_SPARKFFT) {
            std::string line;
            for (uint64_t w = 0; w < nb; ++w) {
                line.assign("\xE2\x94\x82");
                for (size_t b = 0; b < W; ++b) {
                    uint8_t c = out[w * W + b];
                    if (c == 0) line.push_back(' ');
                    else if (c <= 8) { line.push_back((char)0xE2); line.push_back((char)0x96); line.push_back((char)(0x80 + c)); }
                    else bail("index out of bounds: the len is 7 but the index is 7");
                }
                line += "\xE2\x94\x82\n";
                fwrite(line.data(), 1, line.size(), stdout);
            }
        } else if (sink.kind == OP_MARKS) {
            marks.insert(marks.end(), out.begin(), out.begin() + nb);
        } else {
            for (uint64_t w = 0; w < nb; ++w) digits.push_back((char)('0' + out[w]));
        }
    }
    if (sink.kind == OP_BUCKET) printf("%s\n", digits.c_str());
    if (sink.kind == OP_MARKS) print_marks(marks.data(), marks.size(), sink);
}

// do_write (src/lib.rs:178-213).  When the chain is  from [shift] lowpass , or a cascade the library fuses
// (qd_plan_create_stages), the full 0x1000-sample read_at blocks come from ONE fused plan (QD_EPI_CF32_BLOCKS);
// the ragged end of the stream — where every read_at has its own `valid` — and any other chain go through the
// block iterator.
void do_write(const Samples &s, bool overwrite, const std::string &prefix, const ChainSpec *cs) {
    if (prefix == "-") bail("not implemented");
    std::string fn = prefix + ".sr" + std::to_string(s.sample_rate()) + ".cf32";
    int flags = O_WRONLY | (overwrite ? O_CREAT : (O_CREAT | O_EXCL));
    int fd = open(fn.c_str(), flags, 0644);
    if (fd < 0) bail(std::string(strerror(errno)) + " (os error " + std::to_string(errno) + ")");
    uint64_t off = 0, len;
    try { len = s.len(); } catch (...) { close(fd); throw; }
    if (cs && cs->fusable && cs->src->kind == OP_FROM && cs->lowpass && !getenv("QUADRS_HIP_NO_FUSE")) {
        ChainSource in(*cs);
        const MappedFile &data = *in.data;
        qd_chain_desc d;
        std::vector<qd_stage> stages;
        chain_desc(*cs, in, 0x1000, 0x1000, QD_EPI_CF32_BLOCKS, &d, &stages);
        qd_plan *plan = nullptr;
        int rc = create_plan(d, &plan, stages);
        if (rc == QD_OK) {
            qd_plan_info info;
            qd_check(qd_plan_get_info(plan, &info), "plan info");
            if (info.n_windows) {
                std::vector<qd_c32> out(info.n_windows * 0x1000);
                rc = g_gpus > 1 ? qd_plan_run_sharded(plan, data.p, data.mem, out.data(), QD_MEM_HOST)
                                : qd_plan_run(plan, data.p, data.mem, 0, d.n_samples, 0, info.n_windows, out.data(), QD_MEM_HOST, nullptr);
                if (rc == QD_OK) {
                    if (write(fd, out.data(), out.size() * sizeof(qd_c32)) < 0) { qd_plan_destroy(plan); close(fd); bail("write failed"); }
                    off = info.n_windows * 0x1000;
                }
            }
            qd_plan_destroy(plan);
        }
        if (rc != QD_OK && rc != QD_ERR_UNSUPPORTED) { close(fd); qd_check(rc, "fused write"); }
    }
    std::vector<qd_c32> buf(0x1000);
    while (off < len) {
        size_t rd;
        try { rd = s.read_at(off, buf.data(), buf.size()); } catch (...) { close(fd); throw; }
        if (rd == 0) { close(fd); bail("assertion failed: short read at offset " + std::to_string(off) + " of " + std::to_string(len)); }
        off += rd;
        if (write(fd, buf.data(), rd * sizeof(qd_c32)) < 0) { close(fd); bail("write failed"); }
    }
    close(fd);
}

// The `rows` sink: take_fft's rows (src/ffts.rs:18-85) as PREFIX.sr{rate}.w{W}x{count}.pgm — binary PGM, one row per line of the view,
// pixel (norm / 10. * 256.) as u8, the blue channel of the reference's texture (src/eui/mod.rs:104).  A fusable  from [shift] [lowpass]
// chain runs ONE plan (QD_EPI_ROWS_F32) over the mapped file; cascades, and anything the library answers QD_ERR_UNSUPPORTED to, pull
// each row through the iterator chain and hand the rows, side by side, to qd_take_fft.
void do_rows(const Samples &s, const Op &sink, const ChainSpec *cs) {
    const size_t W = sink.width, count = sink.count;
    std::string fn = sink.prefix + ".sr" + std::to_string(s.sample_rate()) + ".w" + std::to_string(W) + "x" + std::to_string(count) + ".pgm";
    int fd = open(fn.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0644);
    if (fd < 0) bail(std::string(strerror(errno)) + " (os error " + std::to_string(errno) + ")");
    std::vector<float> rows(W * count);
    try {
        bool done = false;
        if (cs && cs->fusable && !cs->cascade && cs->src->kind == OP_FROM && !getenv("QUADRS_HIP_NO_FUSE")) {
            ChainSource in(*cs);
            const MappedFile &data = *in.data;
            qd_chain_desc d;
            std::vector<qd_stage> stages;                                    // (stays empty: not a cascade)
            chain_desc(*cs, in, W, 1, QD_EPI_ROWS_F32, &d, &stages);
            qd_rows_desc r{};
            r.struct_size = sizeof r;
            r.has_slice = sink.has_slice ? 1 : 0; r.start = sink.slice_start; r.end = sink.slice_end;
            r.output_len = count; r.windowing = sink.windowing;
            qd_plan *plan = nullptr;
            int rc = qd_plan_create(&d, &plan);
            if (rc == QD_OK) {
                rc = qd_plan_take_fft(plan, &r, data.p, data.mem, 0, d.n_samples, rows.data(), QD_MEM_HOST, nullptr);
                qd_plan_destroy(plan);
                if (rc == QD_OK) done = true;
            }
            if (rc != QD_OK && rc != QD_ERR_UNSUPPORTED) qd_check(rc, "rows");
        }
        if (!done && count) {
            // src/ffts.rs:27-62 over the iterator chain; the rows' samples side by side are a stream whose rows sit at i W
            uint64_t start = sink.slice_start, end = sink.slice_end;
            const uint64_t len = s.len();
            if (!sink.has_slice) { if (len < W) bail("attempt to subtract with overflow"); start = 0; end = len - W; }
            if (!(end > start)) bail("Invalid slice: end (" + std::to_string(end) + ") must be greater than start (" + std::to_string(start) + ")");
            if (!(end < len)) bail("Slice end (" + std::to_string(end) + ") exceeds sample length (" + std::to_string(len) + ")");
            if (!(end - start > count)) bail("Visible samples (" + std::to_string(end - start) + ") must be greater than output length (" + std::to_string(count) + ")");
            if (W < 2) bail("rows -width 1 needs a chain the library fuses");
            const double step = (double)(end - start) / (double)count;
            std::vector<qd_c32> side(W * count);
            for (size_t i = 0; i < count; ++i) {
                const double rr = std::round(step * (double)i);
                const uint64_t ri = !(rr > 0) ? 0 : (rr >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)rr);
                s.read_exact_at(start + ri, side.data() + i * W, W);
            }
            qd_check(qd_take_fft(side.data(), 0, side.size(), (uint64_t)side.size() + 1, 1, 0, (uint64_t)side.size(), W, sink.windowing, count,
                                 rows.data(), QD_MEM_HOST), "take_fft");
        }
    } catch (...) { close(fd); unlink(fn.c_str()); throw; }
    std::string head = "P5\n" + std::to_string(W) + " " + std::to_string(count) + "\n255\n";
    std::vector<uint8_t> px(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) {
        const float v = rows[i] / 10.f * 256.f;                          // `as u8`: saturating, NaN -> 0
        px[i] = !(v > 0.f) ? 0 : (v >= 255.f ? 255 : (uint8_t)v);
    }
    if (write(fd, head.data(), head.size()) < 0 || (px.size() && write(fd, px.data(), px.size()) < 0)) { close(fd); bail("write failed"); }
    close(fd);
}

// The `levels` sink: the qd_summary of the windows sparkfft would print (a cascade's complete windows), as text whose floats (%.9g) parse
// back to the same f32.  A chain the library fuses folds on the device (qd_plan_summarize on a norms plan; with -gpus N one plan per
// window range, merged); every other chain pulls its windows through the iterator chain and folds their norms with qd_summary_fold —
// the same bytes either way.
void print_levels(uint64_t rate, const Op &sink, const qd_summary &sum, const std::vector<float> &peak) {
    printf("levels sample_rate=%" PRIu64 " width=%zu stride=%" PRIu64 " windows=%" PRIu64 "\n", rate, sink.width, sink.stride, (uint64_t)sum.n_windows);
    printf("min %.9g\nmax %.9g\nnan %" PRIu64 "\n", sum.min, sum.max, (uint64_t)sum.n_nan);
    static const char *qname[] = {"q50", "q90", "q99", "q99.9"};
    static const double qval[] = {0.5, 0.9, 0.99, 0.999};
    for (int i = 0; i < 4; ++i) {
        float lo = NAN, hi = NAN;                                         // no values at all: nan nan
        (void)qd_summary_quantile(&sum, qval[i], &lo, &hi);
        printf("%s %.9g %.9g\n", qname[i], lo, hi);
    }
    size_t best = 0;
    for (size_t b = 1; b < peak.size(); ++b) if (peak[b] > peak[best]) best = b;      // the lowest index on ties
    printf("peak_bin %zu %.9g\n", best, peak.empty() ? 0.f : peak[best]);
}

// The fused half of the norms sinks (levels, peaks, means, powers, spreads): one unsharded QD_EPI_NORMS_F32 plan per part (-gpus N; a `gen` source: one), made on
// that part's device.  part(plan, in, g, parts, complete windows, tile) picks its range of the complete windows and runs it; its status is
// checked as `what`.  False when the library has no fused plan for the chain: the caller pulls the windows through the iterator chain.
using NormsPart = std::function<int(qd_plan *plan, ChainSource &in, int g, int parts, uint64_t complete, uint64_t tile)>;
bool norms_fused(const ChainSpec &cs, const Op &sink, const char *what, const NormsPart &part) {
    ChainSource in(cs);
    qd_chain_desc d;
    std::vector<qd_stage> stages;
    chain_desc(cs, in, sink.width, sink.stride, QD_EPI_NORMS_F32, &d, &stages, sink.sink_window);
    int n_dev = 1;
    if (qd_device_count(&n_dev) != QD_OK || n_dev < 1) n_dev = 1;
    const int parts = in.from_gen ? 1 : g_gpus;
    uint64_t complete = 0;
    for (int g = 0; g < parts; ++g) {
        if (parts > 1) qd_check(qd_set_device(g % n_dev), "set device");
        qd_plan *plan = nullptr;
        const int rc = create_plan(d, &plan, stages, 1);
        if (rc == QD_ERR_UNSUPPORTED && g == 0) return false;
        qd_check(rc, "plan");
        if (g == 0) qd_check(qd_plan_complete_windows(plan, &complete), "plan complete windows");
        qd_plan_info info;
        qd_check(qd_plan_get_info(plan, &info), "plan info");
        const int rr = part(plan, in, g, parts, complete, info.tile_windows ? info.tile_windows : 1);
        qd_plan_destroy(plan);
        qd_check(rr, what);
    }
    if (parts > 1) qd_check(qd_set_device(0), "set device");
    return true;
}

bool levels_fused(const ChainSpec &cs, const Op &sink, qd_summary *sum, std::vector<float> *peak, std::vector<float> *floor) {
    return norms_fused(cs, sink, "summarize", [&](qd_plan *plan, ChainSource &in, int g, int parts, uint64_t complete, uint64_t tile) {
        const uint64_t per = ((complete + parts - 1) / parts + tile - 1) / tile * tile;       // tile-aligned ranges, as the library's own shards
        const uint64_t w0 = std::min<uint64_t>(complete, per * g), w1 = std::min<uint64_t>(complete, per * (g + 1));
        qd_summary part;
        std::vector<float> ppeak(sink.width), pfloor(sink.width);
        int mem = QD_MEM_HOST;
        const void *src = w1 > w0 ? in.resident(&mem) : nullptr;
        const int rc = qd_plan_summarize(plan, src, mem, 0, in.n_samples, w0, w1 - w0, &part, ppeak.data(), pfloor.data(), nullptr);
        return rc ? rc : qd_summary_merge(sum, peak->data(), floor->data(), &part, ppeak.data(), pfloor.data());
    });
}

// The iterator half of the norms sinks: the sink's arguments, the windows of sparkfft's loop (src/fft.rs:28-65) ...
void check_norms_sink(const Op &sink) {
    const size_t W = sink.width;
    if (!W || (W & (W - 1))) bail("Radix4 algorithm requires a power-of-two input size");
    if (sink.stride == 0) bail("stride 0 never terminates");
    if (W > 0xffffffffull) bail("width too large");
}
uint64_t spark_windows(const Samples &s, size_t W, uint64_t S) {
    const uint64_t len = s.len();
    if (len < W) bail("attempt to subtract with overflow");
    const uint64_t lim = len - W;
    return lim == 0 ? 0 : (lim - 1) / S + 1;
}
// ... and the norms of its windows [w0, w0 + nb), nb <= kIterBatch: each through read_exact_at, then side by side through a throwaway cf32 norms
// plan.  With stop_short a read that fails ends the batch instead of the program.  Returns the windows whose norms are there.
const uint64_t kIterBatch = 4096;
uint64_t iter_norms(const Samples &s, const Op &sink, uint64_t w0, uint64_t nb, bool stop_short, std::vector<qd_c32> *buf, std::vector<float> *norms) {
    const size_t W = sink.width;
    buf->resize(kIterBatch * W); norms->resize(kIterBatch * W);
    for (uint64_t i = 0; i < nb; ++i) {
        try { s.read_exact_at((w0 + i) * sink.stride, buf->data() + i * W, W); } catch (const Fail &) { if (!stop_short) throw; nb = i; }
    }
    if (!nb) return 0;
    window_gathered(buf->data(), nb, W, sink);
    qd_chain_desc d{};
    d.struct_size = sizeof d;
    d.format = QD_FMT_CF32; d.sample_rate = 1; d.n_samples = nb * W + 1;
    d.width = W; d.stride = W; d.epilogue = QD_EPI_NORMS_F32;
    qd_plan *plan = nullptr;
    qd_check(qd_plan_create(&d, &plan), "plan");
    const int rc = qd_plan_run(plan, buf->data(), QD_MEM_HOST, 0, nb * W, 0, nb, norms->data(), QD_MEM_HOST, nullptr);
    qd_plan_destroy(plan);
    qd_check(rc, "run");
    return nb;
}
// the windows of sparkfft's loop (src/fft.rs:28-65) whose read_exact_at succeeds: a chain's over-reported len fails at the tail
uint64_t readable_windows(const Samples &s, size_t W, uint64_t S, std::vector<qd_c32> *buf) {
    uint64_t nwin = spark_windows(s, W, S);
    buf->resize(W);
    while (nwin) {
        try { s.read_exact_at((nwin - 1) * S, buf->data(), W); break; } catch (const Fail &) { --nwin; }
    }
    return nwin;
}
// a file that must not exist yet: `head`, then `bytes` of data in pieces of 1 GiB
void write_new_file(const std::string &path, const void *data, size_t bytes, const std::string &head = "") {
    int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0644);
    if (fd < 0) bail(std::string(strerror(errno)) + " (os error " + std::to_string(errno) + "): " + path);
    if (!head.empty() && write(fd, head.data(), head.size()) < 0) { close(fd); bail("write failed"); }
    const uint8_t *at = static_cast<const uint8_t *>(data);
    for (size_t left = bytes; left;) {
        const ssize_t w = write(fd, at, std::min<size_t>(left, 1u << 30));
        if (w <= 0) { close(fd); bail("write failed"); }
        at += w; left -= (size_t)w;
    }
    close(fd);
}

void do_levels(const Samples &s, const Op &sink, const ChainSpec *cs) {
    const size_t W = sink.width;
    check_norms_sink(sink);
    qd_summary sum;
    std::vector<float> peak(W), floor(W);
    qd_check(qd_summary_init(&sum, peak.data(), floor.data(), (uint32_t)W), "summary");
    bool done = false;
    if (cs && cs->fusable && !getenv("QUADRS_HIP_NO_FUSE")) done = levels_fused(*cs, sink, &sum, &peak, &floor);
    if (!done) {
        // up to the first window that fails, folded on the host
        const uint64_t nwin = spark_windows(s, W, sink.stride);
        std::vector<qd_c32> buf;
        std::vector<float> norms;
        for (uint64_t w0 = 0; w0 < nwin; w0 += kIterBatch) {
            const uint64_t want = std::min(nwin - w0, kIterBatch), nb = iter_norms(s, sink, w0, want, true, &buf, &norms);
            qd_check(qd_summary_fold(&sum, peak.data(), floor.data(), norms.data(), nb), "fold");
            if (nb < want) break;
        }
    }
    print_levels(s.sample_rate(), sink, sum, peak);
}

// The `peaks` sink: the max-hold picture of the windows sparkfft would print (a cascade's complete windows) as
// PREFIX.sr{rate}.w{W}x{rows}.peak.pgm (and .floor.pgm with -floor yes): row r holds, per bin, the largest (smallest) norm of windows
// [r pool, (r+1) pool).  -pool P, or -count R for pool = max(1, ceil(windows / R)): at most R rows.  Pixels as `rows` (norm / 10 * 256 as
// u8), or with -range lo:hi (v - lo) / (hi - lo) * 256 — the range `levels` tells the user to pass.  A chain the library fuses folds on
// the device (qd_plan_pool on a norms plan; with -gpus N the ROWS are split into contiguous ranges, one plan each); every other chain
// pulls its windows through the iterator chain and folds their norms with qd_pool_fold — the same bytes either way.
//
// The `means` sink is the same picture of the average trace, PREFIX.sr{rate}.w{W}x{rows}.mean.pgm: row r holds, per bin, the mean of the
// norms of its windows, from their exact sum, rounded once (qd_plan_mean fused; qd_mean_fold + qd_mean_finish through the iterator).
// The `powers` sink is the picture of the RMS trace, PREFIX.sr{rate}.w{W}x{rows}.rms.pgm: the root of the mean of the squared norms, from
// their exact sum of squares, rounded once (qd_plan_power fused; qd_power_fold + qd_power_finish through the iterator).
// The `spreads` sink is the picture of the deviation trace, PREFIX.sr{rate}.w{W}x{rows}.std.pgm: the population standard deviation of the
// norms of a row's windows, from their exact sum and sum of squares, rounded once (qd_plan_spread fused; qd_spread_fold + qd_spread_finish
// through the iterator); a NaN norm is ignored, as `means` ignores it.
struct PeakRows {
    uint64_t windows = 0, pool = 1, rows = 0;
    bool mean = false;                            // `means`: peak holds the mean rows, acc the iterator path's exact sums
    bool power = false;                           // `powers`: peak holds the rms rows, acc the iterator path's exact sums of squares
    bool spread = false;                          // `spreads`: peak holds the std rows, acc the iterator path's exact sums and sums of squares
    qd_spread_rows std_at(uint64_t r0, size_t width) { return qd_spread_rows{peak.data() + r0 * width, nullptr, nullptr, nullptr, nullptr}; }
    std::vector<float> peak, floor;
    std::vector<uint64_t> acc;
    void size_for(const Op &sink, uint64_t n) {
        windows = n;
        mean = sink.kind == OP_MEANS;
        power = sink.kind == OP_POWERS;
        spread = sink.kind == OP_SPREADS;
        pool = sink.pool ? sink.pool : std::max<uint64_t>(1, (n + sink.count - 1) / sink.count);
        if (n && pool > n) pool = n;
        rows = n ? (n - 1) / pool + 1 : 0;
        peak.resize(rows * sink.width);
        if (mean || power || spread) return;
        floor.resize(rows * sink.width);
        qd_check(qd_pool_init(peak.data(), floor.data(), (uint32_t)sink.width, rows), "pool init");
    }
    // windows [w0, w1) of the plan, whose first row is r0, into the rows
    int run(qd_plan *plan, const void *src, int mem, uint64_t n_samples, uint64_t w0, uint64_t w1, uint64_t r0, size_t width) {
        if (mean) return qd_plan_mean(plan, src, mem, 0, n_samples, w0, w1 - w0, pool, peak.data() + r0 * width, nullptr, nullptr, QD_MEM_HOST, nullptr);
        if (power) return qd_plan_power(plan, src, mem, 0, n_samples, w0, w1 - w0, pool, peak.data() + r0 * width, nullptr, nullptr, QD_MEM_HOST, nullptr);
        if (spread) { const qd_spread_rows o = std_at(r0, width); return qd_plan_spread(plan, src, mem, 0, n_samples, w0, w1 - w0, pool, &o, QD_MEM_HOST, nullptr); }
        return qd_plan_pool(plan, src, mem, 0, n_samples, w0, w1 - w0, pool, peak.data() + r0 * width, floor.data() + r0 * width, QD_MEM_HOST, nullptr);
    }
};

bool peaks_fused(const ChainSpec &cs, const Op &sink, PeakRows *out) {
    uint64_t rows_per = 0;
    return norms_fused(cs, sink, sink.kind == OP_MEANS ? "mean" : sink.kind == OP_POWERS ? "power" : sink.kind == OP_SPREADS ? "spread" : "pool", [&](qd_plan *plan, ChainSource &in, int g, int parts, uint64_t complete, uint64_t tile) {
        if (g == 0) {
            out->size_for(sink, complete);
            // ranges of whole rows that start on a tile of windows where the pool allows it, as the library's own shards do
            uint64_t a = tile, b = out->pool;
            while (b) { const uint64_t t = a % b; a = b; b = t; }
            const uint64_t q = tile / a;
            rows_per = ((out->rows + parts - 1) / parts + q - 1) / q * q;
        }
        const uint64_t r0 = std::min<uint64_t>(out->rows, rows_per * g), r1 = std::min<uint64_t>(out->rows, rows_per * (g + 1));
        const uint64_t w0 = r0 * out->pool, w1 = std::min<uint64_t>(out->windows, r1 * out->pool);
        if (w1 <= w0) return (int)QD_OK;
        int mem = QD_MEM_HOST;
        const void *src = in.resident(&mem);
        return out->run(plan, src, mem, in.n_samples, w0, w1, r0, sink.width);
    });
}

void do_peaks(const Samples &s, const Op &sink, const ChainSpec *cs) {
    const size_t W = sink.width; const uint64_t S = sink.stride;
    check_norms_sink(sink);
    if (sink.has_range && !(sink.rmax > sink.rmin)) bail(std::string(sink.kind == OP_MEANS ? "means" : sink.kind == OP_POWERS ? "powers" : sink.kind == OP_SPREADS ? "spreads" : "peaks") + " -range takes lo:hi with lo < hi");
    PeakRows pr;
    bool done = false;
    if (cs && cs->fusable && !getenv("QUADRS_HIP_NO_FUSE")) done = peaks_fused(*cs, sink, &pr);
    if (!done) {
        std::vector<qd_c32> buf;
        const uint64_t nwin = readable_windows(s, W, S, &buf);
        pr.size_for(sink, nwin);
        if (pr.mean && pr.rows) {
            pr.acc.resize(pr.rows * W * QD_MEAN_WORDS);
            qd_check(qd_mean_init(pr.acc.data(), (uint32_t)W, pr.rows), "mean init");
        }
        if (pr.power && pr.rows) {
            pr.acc.resize(pr.rows * W * QD_POWER_WORDS);
            qd_check(qd_power_init(pr.acc.data(), (uint32_t)W, pr.rows), "power init");
        }
        if (pr.spread && pr.rows) {
            pr.acc.resize(pr.rows * W * QD_SPREAD_WORDS);
            qd_check(qd_spread_init(pr.acc.data(), (uint32_t)W, pr.rows), "spread init");
        }
        // folded on the host
        std::vector<float> norms;
        for (uint64_t w0 = 0; w0 < nwin; w0 += kIterBatch) {
            const uint64_t nb = iter_norms(s, sink, w0, std::min(nwin - w0, kIterBatch), false, &buf, &norms);
            if (pr.mean) qd_check(qd_mean_fold(pr.acc.data(), (uint32_t)W, pr.pool, w0, norms.data(), nb), "fold");
            else if (pr.power) qd_check(qd_power_fold(pr.acc.data(), (uint32_t)W, pr.pool, w0, norms.data(), nb), "fold");
            else if (pr.spread) qd_check(qd_spread_fold(pr.acc.data(), (uint32_t)W, pr.pool, w0, norms.data(), nb), "fold");
            else qd_check(qd_pool_fold(pr.peak.data(), pr.floor.data(), (uint32_t)W, pr.pool, w0, norms.data(), nb), "fold");
        }
        if (pr.mean && pr.rows) qd_check(qd_mean_finish(pr.acc.data(), (uint32_t)W, pr.rows, pr.peak.data(), nullptr, nullptr), "mean finish");
        if (pr.power && pr.rows) qd_check(qd_power_finish(pr.acc.data(), (uint32_t)W, pr.rows, pr.peak.data(), nullptr, nullptr), "power finish");
        if (pr.spread && pr.rows) { const qd_spread_rows o = pr.std_at(0, W); qd_check(qd_spread_finish(pr.acc.data(), (uint32_t)W, pr.rows, &o), "spread finish"); }
    }
    const std::string stem = sink.prefix + ".sr" + std::to_string(s.sample_rate()) + ".w" + std::to_string(W) + "x" + std::to_string(pr.rows);
    const std::string head = "P5\n" + std::to_string(W) + " " + std::to_string(pr.rows) + "\n255\n";
    const float lo = sink.has_range ? sink.rmin : 0.f, span = sink.has_range ? sink.rmax - sink.rmin : 10.f;
    std::vector<uint8_t> px(pr.peak.size());
    for (int which = 0; which < (sink.want_floor ? 2 : 1); ++which) {
        const std::vector<float> &rows = which ? pr.floor : pr.peak;
        const std::string fn = stem + (pr.mean ? ".mean.pgm" : pr.power ? ".rms.pgm" : pr.spread ? ".std.pgm" : which ? ".floor.pgm" : ".peak.pgm");
        for (size_t i = 0; i < rows.size(); ++i) {
            const float v = (sink.has_range ? rows[i] - lo : rows[i]) / span * 256.f;      // `as u8`: saturating, NaN -> 0
            px[i] = !(v > 0.f) ? 0 : (v >= 255.f ? 255 : (uint8_t)v);
        }
        write_new_file(fn, px.data(), px.size(), head);
    }
}

// The `quantiles` sink: the percentile traces of the windows sparkfft would print (a cascade's complete windows), one picture per -q,
// PREFIX.sr{rate}.w{W}x{rows}.q{Q}.pgm: row r holds, per bin, the lower bound of the level that holds the q-quantile of the norms of windows
// [r pool, (r+1) pool) — q 0.5: the median trace.  The level grid comes from the required -range MIN:MAX: it starts at MIN's bucket of the
// summary's scale (bits >> 20, 8 per octave) and has min(256, MAX's bucket - MIN's bucket + 1) levels; pixels are (v - MIN) / (MAX - MIN) *
// 256 as u8, as `peaks -range`.  A chain the library fuses counts on the device (qd_plan_density on a norms plan; with -gpus N the ROWS are
// split into contiguous ranges, one plan each, each range in spans of rows whose counts fit the library's workspace); every other chain
// pulls its windows through the iterator chain, counts their norms with qd_density_fold and reads them with qd_density_quantile — the
// same bytes either way.
uint32_t level_bucket(float x) { uint32_t b; memcpy(&b, &x, 4); return (b & 0x7fffffffu) >> 20; }

void do_quantiles(const Samples &s, const Op &sink, const ChainSpec *cs) {
    const size_t W = sink.width; const uint64_t S = sink.stride;
    check_norms_sink(sink);
    if (!(sink.rmin >= 0.f) || !(sink.rmax > sink.rmin)) bail("quantiles -range takes lo:hi with 0 <= lo < hi");
    const uint32_t level0 = level_bucket(sink.rmin), L = std::min<uint32_t>(256, level_bucket(sink.rmax) - level0 + 1);
    const size_t nq = sink.qs.size();
    uint64_t windows = 0, pool = 1, rows = 0;
    std::vector<float> traces;                    // nq x rows x W
    auto size_for = [&](uint64_t n) {
        windows = n;
        pool = sink.pool ? sink.pool : std::max<uint64_t>(1, (n + sink.count - 1) / sink.count);
        if (n && pool > n) pool = n;
        rows = n ? (n - 1) / pool + 1 : 0;
        traces.resize(nq * rows * W);
    };
    bool done = false;
    if (cs && cs->fusable && !getenv("QUADRS_HIP_NO_FUSE")) {
        uint64_t rows_per = 0;
        done = norms_fused(*cs, sink, "density", [&](qd_plan *plan, ChainSource &in, int g, int parts, uint64_t complete, uint64_t tile) {
            if (g == 0) {
                size_for(complete);
                uint64_t a = tile, b = pool;
                while (b) { const uint64_t t = a % b; a = b; b = t; }
                const uint64_t q = tile / a;
                rows_per = ((rows + parts - 1) / parts + q - 1) / q * q;
            }
            const uint64_t r0 = std::min<uint64_t>(rows, rows_per * g), r1 = std::min<uint64_t>(rows, rows_per * (g + 1));
            if (r1 <= r0) return (int)QD_OK;
            int mem = QD_MEM_HOST;
            const void *src = in.resident(&mem);
            const uint64_t span = std::max<uint64_t>(1, QD_DENSITY_MAX_WORKSPACE / 4 / L / W);     // rows whose counts fit the workspace
            std::vector<float> part;
            for (uint64_t ra = r0; ra < r1; ra += span) {
                const uint64_t rb = std::min(r1, ra + span), w0 = ra * pool, w1 = std::min<uint64_t>(windows, rb * pool);
                part.resize(nq * (rb - ra) * W);
                const int rc = qd_plan_density(plan, src, mem, 0, in.n_samples, w0, w1 - w0, pool, level0, L, nullptr, sink.qs.data(), (uint32_t)nq,
                                               part.data(), QD_MEM_HOST, nullptr);
                if (rc) return rc;
                for (size_t i = 0; i < nq; ++i)
                    memcpy(traces.data() + (i * rows + ra) * W, part.data() + i * (rb - ra) * W, (rb - ra) * W * sizeof(float));
            }
            return (int)QD_OK;
        });
    }
    if (!done) {
        std::vector<qd_c32> buf;
        const uint64_t nwin = readable_windows(s, W, S, &buf);
        size_for(nwin);
        if (rows) {
            std::vector<uint32_t> counts(rows * W * L);
            qd_check(qd_density_init(counts.data(), (uint32_t)W, L, rows), "density init");
            std::vector<float> norms;
            for (uint64_t w0 = 0; w0 < nwin; w0 += kIterBatch) {
                const uint64_t nb = iter_norms(s, sink, w0, std::min(nwin - w0, kIterBatch), false, &buf, &norms);
                qd_check(qd_density_fold(counts.data(), (uint32_t)W, level0, L, pool, w0, norms.data(), nb), "fold");
            }
            for (size_t i = 0; i < nq; ++i)
                qd_check(qd_density_quantile(counts.data(), (uint32_t)W, level0, L, rows, sink.qs[i], traces.data() + i * rows * W, nullptr, nullptr), "quantile");
        }
    }
    const std::string stem = sink.prefix + ".sr" + std::to_string(s.sample_rate()) + ".w" + std::to_string(W) + "x" + std::to_string(rows);
    const std::string head = "P5\n" + std::to_string(W) + " " + std::to_string(rows) + "\n255\n";
    const float lo = sink.rmin, span = sink.rmax - sink.rmin;
    std::vector<uint8_t> px(rows * W);
    for (size_t i = 0; i < nq; ++i) {
        const std::string fn = stem + ".q" + sink.q_names[i] + ".pgm";
        const float *t = traces.data() + i * rows * W;
        for (size_t k = 0; k < px.size(); ++k) {
            const float v = (t[k] - lo) / span * 256.f;                  // `as u8`: saturating, NaN -> 0
            px[k] = !(v > 0.f) ? 0 : (v >= 255.f ? 255 : (uint8_t)v);
        }
        write_new_file(fn, px.data(), px.size(), head);
    }
}

// The `bands` sink: the band traces of the windows sparkfft would print (a cascade's complete windows), raw little-endian [windows, K]:
// PREFIX.sr{rate}.w{W}.k{K}.level.f32, per window and band the mean of the band's norms from their exact sum, rounded once, and
// PREFIX.sr{rate}.w{W}.k{K}.peak_bin.u32, the lowest fftshifted bin of the band that holds its peak.  One header line on stdout, and with
// -pick one line of digits, the loudest band of each window (0-9a-z, '.' where no band holds a value): what `bucket -by freq K` would print.
// A chain the library fuses folds on the device (qd_plan_bands on a norms plan; with -gpus N the WINDOWS are split into contiguous ranges,
// one plan each, each range in spans of windows whose rows fit the library's workspace); every other chain pulls its windows through the
// iterator chain and folds their norms with qd_bands_fold — the same bytes either way.
void do_bands(const Samples &s, const Op &sink, const ChainSpec *cs) {
    const size_t W = sink.width; const uint64_t S = sink.stride;
    check_norms_sink(sink);
    const uint32_t K = (uint32_t)sink.bands.size();
    uint64_t windows = 0;
    std::vector<float> level;
    std::vector<uint32_t> peak_bin;
    std::vector<uint8_t> pick;
    auto size_for = [&](uint64_t n) { windows = n; level.resize(n * K); peak_bin.resize(n * K); if (sink.pick) pick.resize(n); };
    auto rows_at = [&](uint64_t w) { return qd_band_rows{level.data() + w * K, nullptr, nullptr, nullptr, peak_bin.data() + w * K, sink.pick ? pick.data() + w : nullptr}; };
    bool done = false;
    if (cs && cs->fusable && !getenv("QUADRS_HIP_NO_FUSE")) {
        done = norms_fused(*cs, sink, "bands", [&](qd_plan *plan, ChainSource &in, int g, int parts, uint64_t complete, uint64_t tile) {
            if (g == 0) size_for(complete);
            const uint64_t per = ((complete + parts - 1) / parts + tile - 1) / tile * tile;       // tile-aligned ranges, as the library's own shards
            const uint64_t w0 = std::min<uint64_t>(complete, per * g), w1 = std::min<uint64_t>(complete, per * (g + 1));
            if (w1 <= w0) return (int)QD_OK;
            int mem = QD_MEM_HOST;
            const void *src = in.resident(&mem);
            const uint64_t span = std::max<uint64_t>(1, (1ull << 30) / (16ull * K + 1));          // windows whose rows fit the workspace
            for (uint64_t wa = w0; wa < w1; wa += span) {
                const qd_band_rows rows = rows_at(wa);
                const int rc = qd_plan_bands(plan, src, mem, 0, in.n_samples, wa, std::min(w1, wa + span) - wa, sink.bands.data(), K, &rows, QD_MEM_HOST, nullptr);
                if (rc) return rc;
            }
            return (int)QD_OK;
        });
    }
    if (!done) {
        std::vector<qd_c32> buf;
        const uint64_t nwin = readable_windows(s, W, S, &buf);
        size_for(nwin);
        std::vector<float> norms;
        for (uint64_t w0 = 0; w0 < nwin; w0 += kIterBatch) {
            const uint64_t nb = iter_norms(s, sink, w0, std::min(nwin - w0, kIterBatch), false, &buf, &norms);
            const qd_band_rows rows = rows_at(w0);
            qd_check(qd_bands_fold(norms.data(), (uint32_t)W, nb, sink.bands.data(), K, &rows), "fold");
        }
    }
    const std::string stem = sink.prefix + ".sr" + std::to_string(s.sample_rate()) + ".w" + std::to_string(W) + ".k" + std::to_string(K);
    write_new_file(stem + ".level.f32", level.data(), level.size() * 4);
    write_new_file(stem + ".peak_bin.u32", peak_bin.data(), peak_bin.size() * 4);
    printf("bands width=%zu stride=%llu k=%u windows=%llu\n", W, (unsigned long long)S, K, (unsigned long long)windows);
    if (sink.pick) {
        std::string line(windows, '.');
        for (uint64_t i = 0; i < windows; ++i)
            if (pick[i] < 36) line[i] = "0123456789abcdefghijklmnopqrstuvwxyz"[pick[i]];
        printf("%s\n", line.c_str());
    }
}

// the thresholds of the bursts and emissions sinks: -level X for every bin, or -levels FILE (W raw little-endian f32); -times K multiplies
// each by K in one f32 multiply
std::vector<float> sink_thresholds(const Op &sink, const char *verb) {
    const size_t W = sink.width;
    std::vector<float> thr(W, sink.level);
    if (!sink.has_level) {
        FILE *fp = fopen(sink.levels_file.c_str(), "rb");
        if (!fp) bail(std::string(strerror(errno)) + " (os error " + std::to_string(errno) + "): " + sink.levels_file);
        uint8_t extra;
        const bool ok = fread(thr.data(), 4, W, fp) == W && fread(&extra, 1, 1, fp) == 0;
        fclose(fp);
        if (!ok) bail(std::string(verb) + " -levels takes a file of exactly " + std::to_string(W) + " f32 values (" + std::to_string(W * 4) + " bytes): " + sink.levels_file);
    }
    if (sink.has_times)
        for (float &t : thr) t = t * sink.times;
    return thr;
}

// The `bursts` sink: a threshold per fftshifted bin (-level X for every bin, or -levels FILE: W raw little-endian f32, one row of what
// means, quantiles or peaks write; -times K multiplies each by K in one f32 multiply) applied to the windows sparkfft would print (a
// cascade's complete windows), and the list of the runs of cells at or above it, at least -min windows long, in the order they end:
// PREFIX.sr{rate}.w{W}.bursts holds the first -cap records raw (qd_burst, 32 bytes each), PREFIX.sr{rate}.w{W}.on.u64 the on cells of
// every bin.  One header line on stdout, then with -print N the first N records as `first length bin peak_at peak`.  A chain the library
// fuses lists on the device (qd_plan_bursts on a norms plan); every other chain pulls its windows through the iterator chain into
// qd_bursts_fold and qd_bursts_finish — the same bytes either way.  A run crosses the seam between two devices' ranges, so -gpus N is refused.
struct BurstsVerb {
    using Record = qd_burst;
    static constexpr const char *name = "bursts", *ext = ".bursts";
    static constexpr const char *one_device = "bursts lists one range of windows on one device: a run crosses the seam between two devices' ranges (run it without -gpus)";
    static constexpr size_t words = QD_BURSTS_WORDS, tail = 1;                  // the twin's state: words per bin, and behind them
    std::vector<uint64_t> on;                                                  // the on cells of every bin
    explicit BurstsVerb(const Op &sink) : on(sink.width, 0) {}
    int plan(qd_plan *p, const void *src, int mem, uint64_t n_samples, uint64_t n, const float *thr, const Op &k, Record *list, uint64_t *found) {
        return qd_plan_bursts(p, src, mem, 0, n_samples, 0, n, thr, k.min_len, list, k.cap, found, on.data(), QD_MEM_HOST, nullptr);
    }
    int init(uint64_t *state, uint32_t W) { return qd_bursts_init(state, on.data(), W); }
    int fold(uint64_t *state, uint32_t W, const float *thr, const Op &k, uint64_t at, const float *norms, uint64_t n, Record *list, uint64_t *found) {
        return qd_bursts_fold(state, W, thr, k.min_len, at, norms, n, list, k.cap, found, on.data());
    }
    int finish(uint64_t *state, uint32_t W, const Op &k, Record *list, uint64_t *found) { return qd_bursts_finish(state, W, k.min_len, list, k.cap, found); }
    void more_files(const std::string &stem) const { write_new_file(stem + ".on.u64", on.data(), on.size() * 8); }
    static void header(const Op &k, uint64_t windows, uint64_t found, uint64_t written) {
        printf("bursts width=%zu stride=%llu min=%llu windows=%llu found=%llu written=%llu\n", (size_t)k.width, (unsigned long long)k.stride,
               (unsigned long long)k.min_len, (unsigned long long)windows, (unsigned long long)found, (unsigned long long)written);
    }
    static void print(const Record &b, const Samples &, const Op &) {
        printf("%llu %llu %u %llu %.9g\n", (unsigned long long)b.first, (unsigned long long)b.length, b.bin, (unsigned long long)b.peak_at, (double)b.peak);
    }
};

// The `emissions` sink: the thresholds of `bursts`, and the list of the 4-connected regions of cells at or above them, at least -min
// windows long and -cells cells large, in the order they end: PREFIX.sr{rate}.w{W}.emissions holds the first -cap records raw
// (qd_emission, 56 bytes each).  One header line on stdout, then with -print N the first N records as `first last lo hi cells peak_at
// peak_bin peak flags`, each followed by a line for the reader: start and end in seconds and the low and high edge in Hz relative to the
// chain's centre, (lo - W/2) rate / W and (hi + 1 - W/2) rate / W at the sink's (decimated) rate: what a later `shift` and `lowpass`
// take.  A chain the library fuses lists on the device (qd_plan_emissions on a norms plan); every other chain pulls its windows through
// the iterator chain into qd_emissions_fold and qd_emissions_finish: the same bytes either way.  An emission crosses the seam between
// two devices' ranges, so -gpus N is refused.
struct EmissionsVerb {
    using Record = qd_emission;
    static constexpr const char *name = "emissions", *ext = ".emissions";
    static constexpr const char *one_device = "emissions lists one range of windows on one device: an emission crosses the seam between two devices' ranges (run it without -gpus)";
    static constexpr size_t words = QD_EMISSIONS_WORDS, tail = 2;
    explicit EmissionsVerb(const Op &) {}
    int plan(qd_plan *p, const void *src, int mem, uint64_t n_samples, uint64_t n, const float *thr, const Op &k, Record *list, uint64_t *found) {
        return qd_plan_emissions(p, src, mem, 0, n_samples, 0, n, thr, k.min_len, k.min_cells, list, k.cap, found, QD_MEM_HOST, nullptr);
    }
    int init(uint64_t *state, uint32_t W) { return qd_emissions_init(state, W); }
    int fold(uint64_t *state, uint32_t W, const float *thr, const Op &k, uint64_t at, const float *norms, uint64_t n, Record *list, uint64_t *found) {
        return qd_emissions_fold(state, W, thr, k.min_len, k.min_cells, at, norms, n, list, k.cap, found);
    }
    int finish(uint64_t *state, uint32_t W, const Op &k, Record *list, uint64_t *found) {
        return qd_emissions_finish(state, W, k.min_len, k.min_cells, list, k.cap, found);
    }
    void more_files(const std::string &) const {}
    static void header(const Op &k, uint64_t windows, uint64_t found, uint64_t written) {
        printf("emissions width=%zu stride=%llu min=%llu cells=%llu windows=%llu found=%llu written=%llu\n", (size_t)k.width, (unsigned long long)k.stride,
               (unsigned long long)k.min_len, (unsigned long long)k.min_cells, (unsigned long long)windows, (unsigned long long)found, (unsigned long long)written);
    }
    static void print(const Record &e, const Samples &s, const Op &k) {
        const double rate = (double)s.sample_rate(), W = (double)k.width;
        printf("%llu %llu %u %u %llu %llu %u %.9g %u\n", (unsigned long long)e.first, (unsigned long long)e.last, e.lo, e.hi, (unsigned long long)e.cells,
               (unsigned long long)e.peak_at, e.peak_bin, (double)e.peak, e.flags);
        // a window starts every S samples and holds W of them
        printf("  %.9g s ... %.9g s, %.9g Hz ... %.9g Hz\n", (double)(e.first * k.stride) / rate, (double)(e.last * k.stride + k.width) / rate,
               ((double)e.lo - W / 2) * rate / W, ((double)e.hi + 1 - W / 2) * rate / W);
    }
};

// The body of the list sinks, `bursts` and `emissions`: the fused attempt, else the iterator chain into the twin; the list's file, the
// verb's other files, the header line and the -print records.
template <typename Verb>
void do_list(const Samples &s, const Op &sink, const ChainSpec *cs) {
    using Record = typename Verb::Record;
    const size_t W = sink.width; const uint64_t S = sink.stride;
    check_norms_sink(sink);
    if (g_gpus > 1) bail(Verb::one_device);
    const std::vector<float> thr = sink_thresholds(sink, Verb::name);
    Verb verb(sink);
    std::vector<Record> list(sink.cap);
    Record *lp = sink.cap ? list.data() : nullptr;
    uint64_t found = 0, windows = 0;
    bool done = false;
    if (cs && cs->fusable && !getenv("QUADRS_HIP_NO_FUSE")) {
        done = norms_fused(*cs, sink, Verb::name, [&](qd_plan *plan, ChainSource &in, int, int, uint64_t complete, uint64_t) {
            windows = complete;
            int mem = QD_MEM_HOST;
            const void *src = in.resident(&mem);
            return verb.plan(plan, src, mem, in.n_samples, complete, thr.data(), sink, lp, &found);
        });
    }
    if (!done) {
        std::vector<qd_c32> buf;
        const uint64_t nwin = windows = readable_windows(s, W, S, &buf);
        std::vector<uint64_t> state(Verb::words * W + Verb::tail);
        qd_check(verb.init(state.data(), (uint32_t)W), "init");
        std::vector<float> norms;
        for (uint64_t w0 = 0; w0 < nwin; w0 += kIterBatch) {
            const uint64_t nb = iter_norms(s, sink, w0, std::min(nwin - w0, kIterBatch), false, &buf, &norms);
            qd_check(verb.fold(state.data(), (uint32_t)W, thr.data(), sink, w0, norms.data(), nb, lp, &found), "fold");
        }
        if (nwin == 0) qd_check(verb.fold(state.data(), (uint32_t)W, thr.data(), sink, 0, nullptr, 0, lp, &found), "fold");
        qd_check(verb.finish(state.data(), (uint32_t)W, sink, lp, &found), "finish");
    }
    const uint64_t written = std::min(found, sink.cap);
    const std::string stem = sink.prefix + ".sr" + std::to_string(s.sample_rate()) + ".w" + std::to_string(W);
    write_new_file(stem + Verb::ext, list.data(), (size_t)written * sizeof(Record));
    verb.more_files(stem);
    Verb::header(sink, windows, found, written);
    for (uint64_t i = 0; i < std::min(written, sink.print_n); ++i) Verb::print(list[i], s, sink);
}
void do_bursts(const Samples &s, const Op &sink, const ChainSpec *cs) { do_list<BurstsVerb>(s, sink, cs); }
void do_emissions(const Samples &s, const Op &sink, const ChainSpec *cs) { do_list<EmissionsVerb>(s, sink, cs); }

// The `cuts` sink: the IQ of every record of an emission list (-list FILE.emissions, what `emissions` wrote for the same chain words, -width
// and -stride; -first-window N when the list was made from window N on).  Each record becomes a cut by qd_cut_of_emission (-guard bins on
// either side, an output rate of -oversample x twice the lowpass, -taps, -pad extra outputs on either side): shifted so that the emission
// lands on DC, lowpassed to its width and decimated, always out of the SOURCE samples.  One file PREFIX.NNNNNN.sr{rate / decimate}.cf32
// per record with outputs (NNNNNN the record's place in the list), one header line, and with -print K the first K cuts as
// `shift_hz lowpass_hz decimate taps first count`.  All cuts run in one qd_cuts_run; with QUADRS_HIP_NO_FUSE=1 one by one through
// qd_unpack, qd_shift and qd_lowpass_block: the same bytes.  A cascade has no single shift and decimation to work the cut out from.
// the cuts of a -list file's records (`cuts` and `symbols`): d is the desc of the plan the list came from
void cuts_of_list(const char *verb, const Op &sink, const ChainSpec &cs, const ChainSource &in, qd_chain_desc *d, std::vector<qd_cut> *cuts) {
    FILE *fp = fopen(sink.list_file.c_str(), "rb");
    if (!fp) bail(std::string(strerror(errno)) + " (os error " + std::to_string(errno) + "): " + sink.list_file);
    std::vector<qd_emission> list;
    {
        qd_emission e;
        size_t got;
        while ((got = fread(&e, 1, sizeof e, fp)) == sizeof e) list.push_back(e);
        fclose(fp);
        if (got) bail(std::string(verb) + " -list takes a file of whole qd_emission records (56 bytes each): " + sink.list_file);
    }
    std::vector<qd_stage> stages;
    chain_desc(cs, in, sink.width, sink.stride, QD_EPI_NORMS_F32, d, &stages);
    qd_cut_rule rule{};
    rule.struct_size = sizeof rule;
    rule.guard_bins = (uint32_t)sink.guard; rule.oversample = (uint32_t)sink.oversample; rule.pad = (uint32_t)sink.cut_pad; rule.taps = sink.cut_taps;
    cuts->resize(list.size());
    for (size_t k = 0; k < list.size(); ++k) qd_check(qd_cut_of_emission(d, sink.first_window, &list[k], &rule, &(*cuts)[k]), ("record " + std::to_string(k)).c_str());
}

// cut k of a list through the fine-grained calls (QUADRS_HIP_NO_FUSE=1): qd_unpack | qd_gen, qd_shift, qd_lowpass_block into out[0, count)
void cut_fine(const ChainSource &in, const qd_chain_desc &d, const qd_cut &c, size_t k, qd_c32 *out) {
    static std::vector<qd_c32> raw;
    static std::vector<float> taps;
    const uint64_t pb = qd_pair_bytes(d.format);
    const uint64_t a = c.first * c.decimate, valid = c.count * c.decimate + c.taps;
    raw.resize((size_t)valid);
    if (in.from_gen) qd_check(qd_gen(in.op.cos.data(), in.op.cos.size(), in.op.sample_rate, a, (size_t)valid, raw.data(), QD_MEM_HOST), "gen");
    else qd_check(qd_unpack(d.format, in.data->p + a * pb, (size_t)valid, raw.data(), QD_MEM_HOST), "unpack");
    if (c.shift_hz) qd_check(qd_shift(raw.data(), (size_t)valid, a, qd_shift_ratio(c.shift_hz, d.sample_rate), QD_MEM_HOST), "shift");
    taps.resize((size_t)c.taps);
    qd_check(qd_lowpass_design(c.lowpass_hz, d.sample_rate, (size_t)c.taps, taps.data()), "lowpass_design");
    size_t produced = 0;
    qd_check(qd_lowpass_block(taps.data(), (size_t)c.taps, c.decimate, raw.data(), (size_t)valid, out, (size_t)c.count, &produced, QD_MEM_HOST), "lowpass");
    if (produced != c.count) bail("cut " + std::to_string(k) + ": " + std::to_string(produced) + " outputs, not " + std::to_string(c.count));
}

void do_cuts(const Op &sink, const ChainSpec &cs) {
    if (cs.cascade) bail("cuts takes the chain the list came from as from [shift] [lowpass]: a cascade has no single shift and decimation to place an emission by");
    if (g_gpus > 1) bail("cuts run on one device: every cut reads the one source (run it without -gpus)");
    ChainSource in(cs);
    qd_chain_desc d;
    std::vector<qd_cut> cuts;
    cuts_of_list("cuts", sink, cs, in, &d, &cuts);
    std::vector<uint64_t> offs(cuts.size() + 1);
    uint64_t lo = 0, n = 0;
    qd_check(qd_cuts_geometry(d.sample_rate, d.n_samples, cuts.data(), cuts.size(), offs.data(), &lo, &n), "cuts");
    std::vector<qd_c32> out((size_t)offs[cuts.size()]);
    uint64_t made = 0;
    if (!getenv("QUADRS_HIP_NO_FUSE")) {
        int mem = QD_MEM_HOST;
        const void *src = out.empty() ? nullptr : in.resident(&mem);
        qd_check(qd_cuts_run(d.format, d.sample_rate, d.n_samples, src, mem, 0, d.n_samples, cuts.data(), cuts.size(), out.data(), QD_MEM_HOST, nullptr, nullptr), "cuts");
    } else {
        for (size_t k = 0; k < cuts.size(); ++k)
            if (cuts[k].count) cut_fine(in, d, cuts[k], k, out.data() + offs[k]);
    }
    for (size_t k = 0; k < cuts.size(); ++k) {
        if (!cuts[k].count) continue;
        char num[32];
        snprintf(num, sizeof num, ".%06zu", k);
        write_new_file(sink.prefix + num + ".sr" + std::to_string(d.sample_rate / cuts[k].decimate) + ".cf32", out.data() + offs[k], (size_t)cuts[k].count * sizeof(qd_c32));
        ++made;
    }
    printf("cuts width=%zu stride=%llu first_window=%llu guard=%llu oversample=%llu taps=%llu pad=%llu records=%zu files=%llu samples=%llu\n", (size_t)sink.width,
           (unsigned long long)sink.stride, (unsigned long long)sink.first_window, (unsigned long long)sink.guard, (unsigned long long)sink.oversample,
           (unsigned long long)sink.cut_taps, (unsigned long long)sink.cut_pad, cuts.size(), (unsigned long long)made, (unsigned long long)offs[cuts.size()]);
    for (size_t k = 0; k < std::min<uint64_t>(cuts.size(), sink.print_n); ++k)
        printf("%lld %llu %llu %llu %llu %llu\n", (long long)cuts[k].shift_hz, (unsigned long long)cuts[k].lowpass_hz, (unsigned long long)cuts[k].decimate,
               (unsigned long long)cuts[k].taps, (unsigned long long)cuts[k].first, (unsigned long long)cuts[k].count);
}

// The `symbols` sink: the digit string (-by freq: `bucket -by freq 2`) or the blank / non-blank rows (-by level: sparkfft's rows, the input of
// bits::scan) of every cut of an emission list - `cuts`' words say which cuts, -fft and -step the windows over each cut (at the cut's own
// rate), -range the mark sink's minimum, -window bh a Blackman-Harris window.  PREFIX.symbols holds one line a record,
// `NNNNNN rate windows digits` (digits `-` where the cut has no window), and with -scan SCALE a second one, `NNNNNN bits error`, from
// qd_bits_scan; where bits::scan never returns (QD_ERR_PANIC) that line carries the bits found so far, the error so far and the word
// `loops`: one stuck record does not cost the others.  All of it is ONE qd_cuts_symbols call - the IQ never leaves the device -; with
// QUADRS_HIP_NO_FUSE=1 cut by cut through qd_cuts_run to the host and a plan per cut: the same file.
void do_symbols(const Op &sink, const ChainSpec &cs) {
    if (cs.cascade) bail("symbols takes the chain the list came from as from [shift] [lowpass]: a cascade has no single shift and decimation to place an emission by");
    if (g_gpus > 1) bail("symbols run on one device: every cut reads the one source (run it without -gpus)");
    ChainSource in(cs);
    qd_chain_desc d;
    std::vector<qd_cut> cuts;
    cuts_of_list("symbols", sink, cs, in, &d, &cuts);
    qd_symbols_desc sd{};
    sd.struct_size = sizeof sd;
    sd.epilogue = sink.by_level ? QD_EPI_MARK_U8 : QD_EPI_BUCKET2_U8;
    sd.width = sink.fft; sd.stride = sink.step;
    sd.has_range = sink.has_range ? 1 : 0; sd.range_min = sink.rmin;
    sd.windowing = sink.sink_window;
    std::vector<qd_segment> segs(cuts.size());
    for (size_t k = 0; k < cuts.size(); ++k) segs[k] = qd_segment{0, cuts[k].count};
    std::vector<uint64_t> offs(cuts.size() + 1);
    qd_check(qd_cuts_geometry(d.sample_rate, d.n_samples, cuts.data(), cuts.size(), nullptr, nullptr, nullptr), "symbols");
    qd_check(qd_symbols_geometry(&sd, segs.data(), segs.size(), offs.data()), "symbols");
    std::vector<uint8_t> out((size_t)offs[cuts.size()]);
    if (!getenv("QUADRS_HIP_NO_FUSE")) {
        int mem = QD_MEM_HOST;
        const void *src = out.empty() ? nullptr : in.resident(&mem);
        qd_check(qd_cuts_symbols(d.format, d.sample_rate, d.n_samples, src, mem, 0, d.n_samples, cuts.data(), cuts.size(), &sd, out.data(), QD_MEM_HOST, nullptr, nullptr), "symbols");
    } else {
        std::vector<qd_c32> iq;
        int mem = QD_MEM_HOST;
        const void *src = out.empty() ? nullptr : in.resident(&mem);
        for (size_t k = 0; k < cuts.size(); ++k) {
            const uint64_t nw = offs[k + 1] - offs[k];
            if (!nw) continue;
            iq.resize((size_t)cuts[k].count);
            qd_check(qd_cuts_run(d.format, d.sample_rate, d.n_samples, src, mem, 0, d.n_samples, &cuts[k], 1, iq.data(), QD_MEM_HOST, nullptr, nullptr), "cuts");
            qd_chain_desc w{};
            w.struct_size = sizeof w;
            w.format = QD_FMT_CF32; w.sample_rate = d.sample_rate / cuts[k].decimate; w.n_samples = cuts[k].count;
            w.width = sd.width; w.stride = sd.stride; w.epilogue = sd.epilogue;
            w.has_range = sd.has_range; w.range_min = sd.range_min; w.range_max = 1.0f;
            w.windowing = sd.windowing;
            qd_plan *plan = nullptr;
            qd_check(qd_plan_create(&w, &plan), "plan");
            qd_plan_info info;
            qd_check(qd_plan_get_info(plan, &info), "plan");
            if (info.n_windows != nw) bail("cut " + std::to_string(k) + ": the plan has " + std::to_string(info.n_windows) + " windows, not " + std::to_string(nw));
            qd_check(qd_plan_run(plan, iq.data(), QD_MEM_HOST, 0, cuts[k].count, 0, nw, out.data() + offs[k], QD_MEM_HOST, nullptr), "run");
            qd_plan_destroy(plan);
        }
    }
    std::string text;
    std::vector<uint8_t> bits;
    uint64_t stuck = 0;
    for (size_t k = 0; k < cuts.size(); ++k) {
        const uint64_t nw = offs[k + 1] - offs[k];
        char head[64];
        snprintf(head, sizeof head, "%06zu %llu %llu ", k, (unsigned long long)(d.sample_rate / cuts[k].decimate), (unsigned long long)nw);
        text += head;
        if (!nw) text += '-';
        for (uint64_t w = 0; w < nw; ++w) text.push_back((char)('0' + (out[offs[k] + w] ? 1 : 0)));
        text += '\n';
        if (!sink.has_scan) continue;
        bits.resize((size_t)nw + 1);
        size_t produced = 0;
        double error = 0.0;
        int rc = qd_bits_scan(out.data() + offs[k], (size_t)nw, sink.scan, bits.data(), bits.size(), &produced, &error);
        if (rc == QD_ERR_INVALID && produced > bits.size()) {                // (a scale below 1 emits more bits than marks)
            bits.resize(produced);
            rc = qd_bits_scan(out.data() + offs[k], (size_t)nw, sink.scan, bits.data(), bits.size(), &produced, &error);
        }
        if (rc != QD_ERR_PANIC) qd_check(rc, "scan");                        // the reference's endless loop: what it had found by then
        else ++stuck;
        snprintf(head, sizeof head, "%06zu ", k);
        text += head;
        if (!produced) text += '-';
        for (size_t b = 0; b < produced; ++b) text.push_back((char)('0' + bits[b]));
        snprintf(head, sizeof head, " %.17g", error);
        text += head;
        if (rc == QD_ERR_PANIC) text += " loops";
        text += '\n';
    }
    write_new_file(sink.prefix + ".symbols", text.data(), text.size());
    printf("symbols width=%zu stride=%llu first_window=%llu guard=%llu oversample=%llu taps=%llu pad=%llu fft=%zu step=%llu by=%s window=%s records=%zu windows=%llu",
           (size_t)sink.width, (unsigned long long)sink.stride, (unsigned long long)sink.first_window, (unsigned long long)sink.guard, (unsigned long long)sink.oversample,
           (unsigned long long)sink.cut_taps, (unsigned long long)sink.cut_pad, (size_t)sink.fft, (unsigned long long)sink.step, sink.by_level ? "level" : "freq",
           sink.sink_window ? "bh" : "rect", cuts.size(), (unsigned long long)offs[cuts.size()]);
    if (sink.has_scan) printf(" scan=%.9g stuck=%llu", sink.scan, (unsigned long long)stuck);
    printf("\n");
    size_t at = 0;
    for (uint64_t k = 0; k < sink.print_n && at < text.size(); ++k) {        // -print K: the file's first K lines
        const size_t nl = text.find('\n', at);
        printf("%s\n", text.substr(at, nl - at).c_str());
        at = nl + 1;
    }
}

// The `picture` sink: the waterfall of the windows sparkfft would print (a cascade's complete windows) as the reference's `render` lays
// it out (src/ui/mod.rs:294-412; the colour map is the project's own statement of palette 0.5's HSV -> RGB, include/quadrs_hip.h), written
// as PREFIX.sr{rate}.w{W}.{pxw}x{pxh}.ppm: binary P6, maxval 255, top row first — the buffer as it lies.  A chain the library fuses paints
// on the device (qd_plan_picture on a norms plan).  With -gpus N every device gets a contiguous range of whole strips: the picture of a
// range that starts at strip r0 is the top px_height - r0 row_height rows of the page, so each part paints straight into its rows of
// the one host buffer; marker columns count from the first window of the whole range, so there the parts paint without them and the
// host blackens them.  Every other chain pulls its windows through the iterator chain into qd_picture_fold.  The same bytes either way.
void do_picture(const Samples &s, const Op &sink, const ChainSpec *cs) {
    const size_t W = sink.width; const uint64_t S = sink.stride;
    check_norms_sink(sink);
    qd_picture_desc desc{};
    desc.struct_size = sizeof desc;
    desc.px_width = sink.px_w; desc.px_height = sink.px_h; desc.stretch = sink.stretch; desc.scan = sink.marker; desc.scale = sink.scale;
    uint64_t strips = 0, max_windows = 0, bytes = 0;
    qd_check(qd_picture_geometry(&desc, (uint32_t)W, &strips, &max_windows, &bytes), "picture");
    const uint64_t row_height = (uint64_t)sink.stretch * W + 16;
    const std::string fn = sink.prefix + ".sr" + std::to_string(s.sample_rate()) + ".w" + std::to_string(W) + "." + std::to_string(sink.px_w) + "x" +
                           std::to_string(sink.px_h) + ".ppm";
    int fd = open(fn.c_str(), O_WRONLY | (sink.overwrite ? O_CREAT | O_TRUNC : O_CREAT | O_EXCL), 0644);
    if (fd < 0) bail(std::string(strerror(errno)) + " (os error " + std::to_string(errno) + "): " + fn);
    std::vector<uint8_t> pixels;
    uint64_t painted = 0;
    try {
        pixels.assign((size_t)bytes, 0);
        bool done = false;
        if (cs && cs->fusable && !getenv("QUADRS_HIP_NO_FUSE")) {
            done = norms_fused(*cs, sink, "picture", [&](qd_plan *plan, ChainSource &in, int g, int parts, uint64_t complete, uint64_t) {
                const uint64_t n = std::min(complete, max_windows);
                int mem = QD_MEM_HOST;
                if (parts == 1) {
                    const void *src = n ? in.resident(&mem) : nullptr;
                    return qd_plan_picture(plan, src, mem, 0, in.n_samples, 0, n, &desc, pixels.data(), QD_MEM_HOST, &painted, nullptr);
                }
                painted = n;
                const uint64_t used = (n + sink.px_w - 1) / sink.px_w, per = (used + parts - 1) / parts;      // strips that hold a window; a part's share
                const uint64_t r0 = per * g, w0 = r0 * sink.px_w, w1 = std::min(n, (r0 + per) * sink.px_w);
                if (w1 <= w0 || r0 * row_height >= sink.px_h) return (int)QD_OK;                      // no windows, or the strip at oy == h
                qd_picture_desc part = desc;
                part.px_height = (uint32_t)(sink.px_h - r0 * row_height);
                part.scan = 0;
                return qd_plan_picture(plan, in.resident(&mem), mem, 0, in.n_samples, w0, w1 - w0, &part, pixels.data(), QD_MEM_HOST, nullptr, nullptr);
            });
            if (done && g_gpus > 1 && sink.marker) {
                for (uint64_t p = 0; p < painted; p += sink.marker) {
                    const uint64_t x = p % sink.px_w, oy = p / sink.px_w * row_height;
                    for (uint64_t y = oy; y < oy + (uint64_t)sink.stretch * W && y < sink.px_h; ++y) memset(pixels.data() + ((sink.px_h - 1 - y) * sink.px_w + x) * 3, 0, 3);
                }
            }
        }
        if (!done) {
            std::vector<qd_c32> buf;
            painted = std::min(readable_windows(s, W, S, &buf), max_windows);
            std::vector<float> norms;
            for (uint64_t w0 = 0; w0 < painted; w0 += kIterBatch) {
                const uint64_t nb = iter_norms(s, sink, w0, std::min(painted - w0, kIterBatch), false, &buf, &norms);
                qd_check(qd_picture_fold(pixels.data(), &desc, (uint32_t)W, w0, norms.data(), nb), "fold");
            }
        }
        const std::string head = "P6\n" + std::to_string(sink.px_w) + " " + std::to_string(sink.px_h) + "\n255\n";
        if (write(fd, head.data(), head.size()) < 0) bail("write failed");
        const uint8_t *at = pixels.data();
        for (size_t left = pixels.size(); left;) {
            const ssize_t w = write(fd, at, std::min<size_t>(left, 1u << 30));
            if (w <= 0) bail("write failed");
            at += w; left -= (size_t)w;
        }
    } catch (...) { close(fd); unlink(fn.c_str()); throw; }
    close(fd);
    printf("picture width=%zu stride=%llu size=%ux%u stretch=%u scan=%u scale=%.9g strips=%llu max_windows=%llu painted=%llu\n", W, (unsigned long long)S,
           sink.px_w, sink.px_h, sink.stretch, sink.marker, sink.scale, (unsigned long long)strips, (unsigned long long)max_windows, (unsigned long long)painted);
}

void usage() {
    fprintf(stderr,
            "usage: quadrs-hip [-gpus N] \\\n"
            "    from [-sr SAMPLE_RATE] [-format cf32|cs8|cu8|cs16] FILENAME.sr32k.cf32 \\\n"
            "   shift [-]FREQUENCY \\\n"
            " lowpass [-power 20] [-decimate 8] FREQUENCY \\\n"
            "sparkfft [-width 128] [-stride =width] [-range MIN:MAX] \\\n"
            "  bucket [-width 128] [-stride =width] -by freq COUNT \\\n"
            "   marks [-width 128] [-stride =width] [-min 0.08] [-scan SCALE] \\\n"
            "  levels [-width 128] [-stride =width] \\\n"
            "   peaks [-width 128] [-stride =width] (-pool WINDOWS | -count 2048) [-range MIN:MAX] [-floor no] FILENAME_PREFIX \\\n"
            "   means [-width 128] [-stride =width] (-pool WINDOWS | -count 2048) [-range MIN:MAX] FILENAME_PREFIX \\\n"
            "   powers [-width 128] [-stride =width] (-pool WINDOWS | -count 2048) [-range MIN:MAX] FILENAME_PREFIX \\\n"
            "  spreads [-width 128] [-stride =width] (-pool WINDOWS | -count 2048) [-range MIN:MAX] FILENAME_PREFIX \\\n"
            "quantiles [-width 128] [-stride =width] (-pool WINDOWS | -count 2048) -q 0.5[,0.9,...] -range MIN:MAX FILENAME_PREFIX \\\n"
            "   bands [-width 128] [-stride =width] (-bins LO:HI[,LO:HI...] | -split K) [-pick] FILENAME_PREFIX \\\n"
            "  bursts [-width 128] [-stride =width] (-level X | -levels FILE) [-times K] [-min 1] [-cap 1048576] [-print 0] FILENAME_PREFIX \\\n"
            "emissions [-width 128] [-stride =width] (-level X | -levels FILE) [-times K] [-min 1] [-cells 1] [-cap 1048576] [-print 0] FILENAME_PREFIX \\\n"
            "    cuts -width W [-stride =width] -list FILE.emissions [-first-window 0] [-guard 1] [-oversample 2] [-taps 0] [-pad 1] [-print 0] FILENAME_PREFIX \\\n"
            " symbols -width W [-stride =width] -list FILE.emissions [cuts' flags] -fft w [-step =w] -by freq|level [-range min] [-window bh|rect] \\\n"
            "         [-scan SCALE] [-print 0] FILENAME_PREFIX \\\n"
            " picture [-width 8] [-stride 1] -size PXWxPXH [-stretch 4] [-scan 0] [-scale 2.29] [-overwrite no] FILENAME_PREFIX \\\n"
            "    rows [-width 512] [-count 2048] [-slice START:END] [-window bh|rect] FILENAME_PREFIX \\\n"
            "   write [-overwrite no] FILENAME_PREFIX \\\n"
            "     gen [-cos FREQUENCY]* [-len 1 (second)] SAMPLE_RATE \\\n"
            "\nsparkfft, bucket, marks, levels, peaks, means, powers, spreads, quantiles, emissions, bands, bursts and picture also take [-window bh|rect] (default rect):\n"
            "a Blackman-Harris window on every window's samples in front of the transform\n"
            "\n\nFormat for FREQUENCY, SAMPLE_RATE, and other suffixes: 123, 123k, 123M, 123G\n");
}

}  // namespace

int main(int argc, char **argv) {
    std::vector<std::string> args(argv + 1, argv + argc);
    try {
        // engine option in front of the reference's grammar: -gpus N shards the sink's windows over N devices in this process
        if (args.size() >= 2 && args[0] == "-gpus") {
            g_gpus = atoi(args[1].c_str());
            if (g_gpus < 1 || g_gpus > QD_MAX_SHARDS) { usage(); fprintf(stderr, "Error: -gpus takes 1..%d\n", QD_MAX_SHARDS); return 2; }
            args.erase(args.begin(), args.begin() + 2);
        }
        // -parse-only: print what the grammar (src/args.rs) made of the command line, one operation per line, and stop before
        // any file or device is touched (tests: filename -> (sample rate, format) guessing, defaults, SI suffixes)
        bool parse_only = false;
        if (!args.empty() && args[0] == "-parse-only") { parse_only = true; args.erase(args.begin()); }
        if (args.empty()) { usage(); return 2; }
        std::vector<Op> ops;
        try { ops = parse(args); } catch (const Fail &f) { usage(); fprintf(stderr, "Error: %s\n", f.msg.c_str()); return 2; }
        if (parse_only) {
            static const char *fmt_name[] = {"cf32", "cs8", "cu8", "cs16"};
            for (const Op &op : ops) {
                switch (op.kind) {
                case OP_FROM: printf("from file=%s sample_rate=%llu format=%s\n", op.filename.c_str(), (unsigned long long)op.sample_rate, fmt_name[op.format & 3]); break;
                case OP_GEN: printf("gen cos=%zu sample_rate=%llu seconds=%.17g\n", op.cos.size(), (unsigned long long)op.sample_rate, op.seconds); break;
                case OP_SHIFT: printf("shift %lld\n", (long long)op.shift); break;
                case OP_LOWPASS: printf("lowpass frequency=%llu decimate=%llu size=%zu\n", (unsigned long long)op.lp_freq, (unsigned long long)op.decimate, op.size); break;
                case OP_SPARKFFT: printf("sparkfft width=%zu stride=%llu range=%s\n", op.width, (unsigned long long)op.stride, op.has_range ? "yes" : "no"); break;
                case OP_BUCKET: printf("bucket width=%zu stride=%llu levels=%zu\n", op.width, (unsigned long long)op.stride, op.levels); break;
                case OP_MARKS: printf("marks width=%zu stride=%llu min=%s scan=%s\n", op.width, (unsigned long long)op.stride, op.has_range ? "yes" : "no", op.has_scan ? "yes" : "no"); break;
                case OP_LEVELS: printf("levels width=%zu stride=%llu\n", op.width, (unsigned long long)op.stride); break;
                case OP_PEAKS:
                    printf("peaks width=%zu stride=%llu %s=%llu range=%s floor=%d\n", op.width, (unsigned long long)op.stride, op.pool ? "pool" : "count",
                           (unsigned long long)(op.pool ? op.pool : op.count), op.has_range ? "yes" : "no", op.want_floor ? 1 : 0);
                    break;
                case OP_MEANS:
                case OP_POWERS:
                case OP_SPREADS:
                    printf("%s width=%zu stride=%llu %s=%llu range=%s\n", op.kind == OP_MEANS ? "means" : op.kind == OP_POWERS ? "powers" : "spreads", op.width, (unsigned long long)op.stride, op.pool ? "pool" : "count",
                           (unsigned long long)(op.pool ? op.pool : op.count), op.has_range ? "yes" : "no");
                    break;
                case OP_QUANTILES: {
                    std::string qs;
                    for (const std::string &q : op.q_names) qs += (qs.empty() ? "" : ",") + q;
                    printf("quantiles width=%zu stride=%llu %s=%llu q=%s range=%.9g:%.9g\n", op.width, (unsigned long long)op.stride, op.pool ? "pool" : "count",
                           (unsigned long long)(op.pool ? op.pool : op.count), qs.c_str(), op.rmin, op.rmax);
                    break;
                }
                case OP_BANDS: {
                    std::string bs;
                    for (const qd_band &b : op.bands) bs += (bs.empty() ? "" : ",") + std::to_string(b.lo) + ":" + std::to_string(b.hi);
                    printf("bands width=%zu stride=%llu k=%zu bins=%s pick=%d\n", op.width, (unsigned long long)op.stride, op.bands.size(), bs.c_str(), op.pick ? 1 : 0);
                    break;
                }
                case OP_BURSTS:
                    if (op.has_level) printf("bursts width=%zu stride=%llu level=%.9g", op.width, (unsigned long long)op.stride, op.level);
                    else printf("bursts width=%zu stride=%llu levels=%s", op.width, (unsigned long long)op.stride, op.levels_file.c_str());
                    printf(" times=%.9g min=%llu cap=%llu print=%llu\n", op.times, (unsigned long long)op.min_len, (unsigned long long)op.cap, (unsigned long long)op.print_n);
                    break;
                case OP_EMISSIONS:
                    if (op.has_level) printf("emissions width=%zu stride=%llu level=%.9g", op.width, (unsigned long long)op.stride, op.level);
                    else printf("emissions width=%zu stride=%llu levels=%s", op.width, (unsigned long long)op.stride, op.levels_file.c_str());
                    printf(" times=%.9g min=%llu cells=%llu cap=%llu print=%llu\n", op.times, (unsigned long long)op.min_len, (unsigned long long)op.min_cells,
                           (unsigned long long)op.cap, (unsigned long long)op.print_n);
                    break;
                case OP_CUTS:
                    printf("cuts width=%zu stride=%llu list=%s first_window=%llu guard=%llu oversample=%llu taps=%llu pad=%llu print=%llu\n", op.width, (unsigned long long)op.stride,
                           op.list_file.c_str(), (unsigned long long)op.first_window, (unsigned long long)op.guard, (unsigned long long)op.oversample,
                           (unsigned long long)op.cut_taps, (unsigned long long)op.cut_pad, (unsigned long long)op.print_n);
                    break;
                case OP_SYMBOLS:
                    printf("symbols width=%zu stride=%llu list=%s first_window=%llu guard=%llu oversample=%llu taps=%llu pad=%llu fft=%zu step=%llu by=%s", op.width,
                           (unsigned long long)op.stride, op.list_file.c_str(), (unsigned long long)op.first_window, (unsigned long long)op.guard,
                           (unsigned long long)op.oversample, (unsigned long long)op.cut_taps, (unsigned long long)op.cut_pad, op.fft, (unsigned long long)op.step,
                           op.by_level ? "level" : "freq");
                    if (op.has_range) printf(" range=%.9g", op.rmin);
                    if (op.has_scan) printf(" scan=%.9g", op.scan);
                    printf(" print=%llu\n", (unsigned long long)op.print_n);
                    break;
                case OP_PICTURE:
                    printf("picture width=%zu stride=%llu size=%ux%u stretch=%u scan=%u scale=%.9g overwrite=%d\n", op.width, (unsigned long long)op.stride, op.px_w, op.px_h,
                           op.stretch, op.marker, op.scale, op.overwrite ? 1 : 0);
                    break;
                case OP_WRITE: printf("write prefix=%s overwrite=%d\n", op.prefix.c_str(), op.overwrite ? 1 : 0); break;
                case OP_ROWS:
                    printf("rows width=%zu count=%zu slice=%s window=%s\n", op.width, op.count,
                           op.has_slice ? (std::to_string(op.slice_start) + ":" + std::to_string(op.slice_end)).c_str() : "all", op.windowing ? "bh" : "rect");
                    break;
                }
                if (op.sink_window) printf("window=bh\n");      // the verb above was given -window bh
            }
            return 0;
        }

        // fold the commands left to right (src/bin/quadrs.rs:48-56)
        std::unique_ptr<Samples> samples;
        ChainSpec cs;
        bool chain_clean = true;        // from [shift] [lowpass] so far, each at most once, in that order (else: a cascade)
        for (size_t i = 0; i < ops.size(); ++i) {
            const Op &op = ops[i];
            switch (op.kind) {
            case OP_FROM:
                samples.reset(new SampleFile(op.filename, op.format, op.sample_rate));
                cs = ChainSpec{}; cs.src = &op; cs.fusable = true; chain_clean = true;
                break;
            case OP_GEN:
                samples.reset(new Gen(op.cos, op.sample_rate, op.seconds));
                cs = ChainSpec{}; cs.src = &op; cs.fusable = true; chain_clean = true;
                break;
            case OP_SHIFT:
                if (!samples) bail("shift requires an input");
                if (cs.shift || cs.lowpass) chain_clean = false;
                samples.reset(new Shift(std::move(samples), op.shift));
                cs.shift = &op;
                cs.stages.push_back(&op);
                break;
            case OP_LOWPASS:
                if (!samples) bail("lowpass requires an input");
                if (cs.lowpass) chain_clean = false;
                samples.reset(new LowPass(std::move(samples), op.lp_freq, op.decimate, op.size));
                cs.lowpass = &op;
                cs.stages.push_back(&op);
                break;
            case OP_SPARKFFT:
            case OP_BUCKET:
            case OP_MARKS:
                if (!samples) bail(op.kind == OP_SPARKFFT ? "sparkfft requires an input" : op.kind == OP_MARKS ? "marks requires an input" : "bucket -by freq requires an input");
                if (op.kind == OP_BUCKET && op.levels != 2) bail("only supporting two levels for now");
                if (cs.fusable && !getenv("QUADRS_HIP_NO_FUSE")) {
                    cs.cascade = !chain_clean;
                    if (!run_fused(cs, op, *samples)) run_iter_sink(*samples, op, true);
                } else run_iter_sink(*samples, op);
                break;
            case OP_LEVELS:
                if (!samples) bail("levels requires an input");
                cs.cascade = !chain_clean;
                do_levels(*samples, op, &cs);
                break;
            case OP_SPREADS:
            case OP_POWERS:
            case OP_MEANS:
            case OP_PEAKS:
                if (!samples) bail(std::string(op.kind == OP_SPREADS ? "spreads" : op.kind == OP_POWERS ? "powers" : op.kind == OP_MEANS ? "means" : "peaks") + " requires an input");
                cs.cascade = !chain_clean;
                do_peaks(*samples, op, &cs);
                break;
            case OP_QUANTILES:
                if (!samples) bail("quantiles requires an input");
                cs.cascade = !chain_clean;
                do_quantiles(*samples, op, &cs);
                break;
            case OP_BANDS:
                if (!samples) bail("bands requires an input");
                cs.cascade = !chain_clean;
                do_bands(*samples, op, &cs);
                break;
            case OP_BURSTS:
                if (!samples) bail("bursts requires an input");
                cs.cascade = !chain_clean;
                do_bursts(*samples, op, &cs);
                break;
            case OP_EMISSIONS:
                if (!samples) bail("emissions requires an input");
                cs.cascade = !chain_clean;
                do_emissions(*samples, op, &cs);
                break;
            case OP_CUTS:
                if (!samples) bail("cuts requires an input");
                cs.cascade = !chain_clean;
                do_cuts(op, cs);
                break;
            case OP_SYMBOLS:
                if (!samples) bail("symbols requires an input");
                cs.cascade = !chain_clean;
                do_symbols(op, cs);
                break;
            case OP_PICTURE:
                if (!samples) bail("picture requires an input");
                cs.cascade = !chain_clean;
                do_picture(*samples, op, &cs);
                break;
            case OP_ROWS:
                if (!samples) bail("rows requires an input");
                cs.cascade = !chain_clean;
                do_rows(*samples, op, &cs);
                break;
            case OP_WRITE:
                if (!samples) bail("write requires an input");
                cs.cascade = !chain_clean;
                do_write(*samples, op.overwrite, op.prefix, &cs);
                break;
            }
        }
        return 0;
    } catch (const Fail &f) {
        fflush(stdout);
        fprintf(stderr, "Error: %s\n", f.msg.c_str());
        return 1;
    }
}
