// bed_lite.hpp — BED text into intervals, as a push parser: feed(bytes, n) as the file comes, then finish().  What
// fadehip_intervals_load_bed reads a RepeatMasker BED with, and what the driver's --repeats checks its path with (plain C++,
// no device; build/bed_selftest holds it to hand cases under ASan + UBSan).  The rule:
//
//   lines    end at '\n'; a '\r' in front of it is dropped; the last line may lack its '\n'
//   skipped  empty lines, and lines that start with '#', "track" or "browser"
//   fields   separated by tabs, at least three; what follows the third is ignored
//   name     1 to 255 bytes, taken as they stand; names get their ids in order of first appearance
//   start    decimal digits only; 0 <= start < end <= 2^31 - 1 (0-based, half-open)
//   errors   anything else stops the parse: error() names the 1-based line
//
// Intervals are handed on in pieces of at most `piece` — the sink sees every name an interval of the piece uses in names()
// before it sees the piece — and of a line only its first KEEP bytes are held, so a file of millions of lines never stands in
// memory as text.
#pragma once
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

namespace fadehip {
namespace bed {

constexpr int64_t MAX_END = 0x7fffffffll;  // 2^31 - 1
constexpr size_t MAX_NAME = 255;
constexpr size_t KEEP = 512;  // bytes of a line that are held: the three fields fit (255 + two numbers) with room for leading zeros

// why `path` cannot be read as BED text, or "": compressed files are refused by name (plain text only)
inline std::string path_refusal(const std::string &path) {
    const auto ends = [&](const char *suf) {
        const size_t n = strlen(suf);
        return path.size() >= n && path.compare(path.size() - n, n, suf) == 0;
    };
    if (ends(".gz") || ends(".bgz")) return "the BED file is read as plain text: not a compressed file (" + path + "); decompress it first";
    return "";
}

class Parser {
public:
    // a piece: n intervals as three arrays; false stops the parse with sink_error as the message
    using Sink = std::function<bool(const int32_t *chrom, const int64_t *start, const int64_t *end, size_t n, std::string &sink_error)>;

    explicit Parser(Sink sink, size_t piece = (size_t)1 << 18) : sink_(std::move(sink)), piece_(piece ? piece : 1) {}

    bool feed(const void *bytes, size_t n) {
        if (failed_) return false;
        const char *p = (const char *)bytes;
        for (size_t k = 0; k < n; k++) {
            const char c = p[k];
            if (c == '\n') {
                if (!end_line()) return false;
                continue;
            }
            if (kept_.size() < KEEP) kept_ += c;
            else if (over_n_++ == 0) over_first_ = c;
            last_ = c;
            any_ = true;
        }
        return true;
    }

    bool finish() {
        if (failed_) return false;
        if (finished_) return true;
        if (any_ && !end_line()) return false;
        if (!flush()) return false;
        finished_ = true;
        return true;
    }

    const std::vector<std::string> &names() const { return names_; }
    const std::string &error() const { return err_; }
    uint64_t n_intervals() const { return total_; }
    uint64_t n_lines() const { return line_; }

private:
    bool fail(const std::string &what) {
        err_ = "line " + std::to_string(line_) + ": " + what;
        failed_ = true;
        return false;
    }

    static bool number(const char *b, size_t n, int64_t *v) {
        if (!n) return false;
        int64_t x = 0;
        for (size_t k = 0; k < n; k++) {
            if (b[k] < '0' || b[k] > '9') return false;
            x = x * 10 + (b[k] - '0');
            if (x > MAX_END) x = MAX_END + 1;  // (beyond the bounds already: no overflow whatever follows)
        }
        *v = x;
        return true;
    }

    bool flush() {
        if (chrom_.empty()) return true;
        std::string why;
        if (!sink_(chrom_.data(), start_.data(), end_.data(), chrom_.size(), why)) {
            err_ = why;
            failed_ = true;
            return false;
        }
        chrom_.clear();
        start_.clear();
        end_.clear();
        return true;
    }

    // the line that has just ended (at '\n', or at the end of the input)
    bool end_line() {
        line_++;
        size_t n = kept_.size();
        size_t over = over_n_;
        if (any_ && last_ == '\r') {  // the '\r' in front of the line's end is dropped, wherever it was counted
            if (over) over--;
            else n--;
        }
        const char *b = kept_.data();
        const bool skip = n == 0 || b[0] == '#' || (n >= 5 && memcmp(b, "track", 5) == 0) || (n >= 7 && memcmp(b, "browser", 7) == 0);
        bool ok = true;
        if (!skip) ok = take(b, n, over);
        kept_.clear();
        over_n_ = 0;
        over_first_ = 0;
        last_ = 0;
        any_ = false;
        return ok;
    }

    bool take(const char *b, size_t n, size_t over) {
        size_t t1 = 0;
        while (t1 < n && b[t1] != '\t') t1++;
        size_t t2 = t1 + 1;
        while (t2 < n && b[t2] != '\t') t2++;
        if (t1 >= n || t2 >= n) {
            if (over) return fail("the first three fields take more than " + std::to_string(KEEP) + " bytes");
            return fail("fewer than three tab-separated fields");
        }
        size_t t3 = t2 + 1;
        while (t3 < n && b[t3] != '\t') t3++;
        if (t3 >= n && over && over_first_ != '\t') return fail("the first three fields take more than " + std::to_string(KEEP) + " bytes");
        if (t1 == 0) return fail("the name is empty");
        if (t1 > MAX_NAME) return fail("the name is longer than " + std::to_string(MAX_NAME) + " bytes");
        int64_t s = 0, e = 0;
        if (!number(b + t1 + 1, t2 - t1 - 1, &s)) return fail("start is not a number of decimal digits");
        if (!number(b + t2 + 1, t3 - t2 - 1, &e)) return fail("end is not a number of decimal digits");
        if (e > MAX_END) return fail("end is beyond 2^31 - 1");
        if (s >= e) return fail("start is not below end");
        const std::string name(b, t1);
        auto it = ids_.find(name);
        if (it == ids_.end()) {
            it = ids_.emplace(name, (int32_t)names_.size()).first;
            names_.push_back(name);
        }
        chrom_.push_back(it->second);
        start_.push_back(s);
        end_.push_back(e);
        total_++;
        return chrom_.size() < piece_ || flush();
    }

    Sink sink_;
    size_t piece_;
    std::string kept_;      // the line so far, its first KEEP bytes
    size_t over_n_ = 0;     // bytes of it beyond those ...
    char over_first_ = 0;   // ... and the first of them
    char last_ = 0;         // the line's last byte so far
    bool any_ = false;      // the line has bytes
    uint64_t line_ = 0, total_ = 0;
    bool failed_ = false, finished_ = false;
    std::string err_;
    std::vector<std::string> names_;
    std::unordered_map<std::string, int32_t> ids_;
    std::vector<int32_t> chrom_;
    std::vector<int64_t> start_, end_;
};

}  // namespace bed
}  // namespace fadehip
