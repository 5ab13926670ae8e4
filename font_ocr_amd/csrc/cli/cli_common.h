// What the `ncc` and `focr` command lines share: clap-shaped argument mechanics, the two ways to end the program,
// UTF-8 and the --verify file name.  Header-only, standard library only.
#pragma once

#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <unistd.h>

namespace cli {

// clap's usage error: the message, the program's "Usage: ..." line, exit code 2
[[noreturn]] inline void usage_error(const char *usage_line, const std::string &msg) {
    fprintf(stderr, "error: %s\n\n%s\n\nFor more information, try '--help'.\n", msg.c_str(), usage_line);
    exit(2);
}

[[noreturn]] inline void die(const char *program, const std::string &msg, int code) {
    fprintf(stderr, "%s: %s\n", program, msg.c_str());
    // _exit, not exit: once a device is in use, worker threads may be inside HIP calls, and running the HIP runtime's
    // atexit handlers / static destructors under them can hang or crash instead of returning the code
    fflush(stdout);
    fflush(stderr);
    _exit(code);
}

// Rust's u32::from_str, which clap applies in the reference: an optional '+', then decimal digits only, at most u32::MAX
inline bool parse_u32(const std::string &s, uint32_t *out) {
    size_t i = !s.empty() && s[0] == '+' ? 1 : 0;
    if (i == s.size()) return false;
    uint64_t r = 0;
    for (; i < s.size(); i++) {
        if (s[i] < '0' || s[i] > '9') return false;
        r = r * 10 + (uint64_t)(s[i] - '0');
        if (r > 0xffffffffull) return false;
    }
    *out = (uint32_t)r;
    return true;
}

inline bool parse_f32(const std::string &s, float *out) {
    char *e = nullptr;
    *out = strtof(s.c_str(), &e);
    return e && !*e && !s.empty();
}

// Walks argv as clap does: `--key=value`, `--key value`, the glued short forms `-t13` and `-t=13`.  The program keeps its
// own `if (key == ...)` chain; a value that is missing or malformed is a usage error here.
class ArgCursor {
public:
    std::string key;  // the flag of the current argument, without its value
    std::string val;  // its value, once need() was called
    std::string raw;  // the current argument as typed

    ArgCursor(int argc, char **argv, const char *usage_line) : v_(argv + 1, argv + argc), usage_(usage_line) {}

    bool next() {
        if (i_ >= v_.size()) return false;
        raw = key = v_[i_++];
        val.clear();
        has_val_ = false;
        if (key.rfind("--", 0) == 0) {
            const size_t eq = key.find('=');
            if (eq != std::string::npos) {
                val = key.substr(eq + 1);
                key = key.substr(0, eq);
                has_val_ = true;
            }
        } else if (key.size() > 2 && key[0] == '-' && key[1] != '-') {  // -t13, -ipage.pgm
            val = key.substr(key[2] == '=' ? 3 : 2);
            key = key.substr(0, 2);
            has_val_ = true;
        }
        return true;
    }
    const std::string &need() {
        if (!has_val_) {
            if (i_ >= v_.size()) fail("a value is required for '" + key + "' but none was supplied");
            val = v_[i_++];
            has_val_ = true;
        }
        return val;
    }
    void need_all(std::vector<std::string> &out) {  // num_args = 1..: every following argument that is not an option
        out.push_back(need());
        while (i_ < v_.size() && !is_opt(v_[i_])) out.push_back(v_[i_++]);
    }
    uint32_t u32() {
        uint32_t r = 0;
        if (!parse_u32(need(), &r)) invalid();
        return r;
    }
    uint32_t u32_at_most(uint32_t limit, const char *why) {
        const uint32_t r = u32();
        if (r > limit) invalid(std::string(": ") + why);
        return r;
    }
    float f32() {
        float r = 0.f;
        if (!parse_f32(need(), &r)) invalid();
        return r;
    }
    [[noreturn]] void invalid(const std::string &why = "") { fail("invalid value '" + val + "' for '" + key + "'" + why); }
    [[noreturn]] void unexpected() { fail("unexpected argument '" + raw + "' found"); }
    [[noreturn]] void fail(const std::string &msg) { usage_error(usage_, msg); }

private:
    static bool is_opt(const std::string &s) { return s.size() > 1 && s[0] == '-' && !(isdigit((unsigned char)s[1]) || s[1] == '.'); }
    std::vector<std::string> v_;
    const char *usage_;
    size_t i_ = 0;
    bool has_val_ = false;
};

inline std::vector<uint32_t> utf8_decode(const std::string &s) {
    std::vector<uint32_t> out;
    for (size_t i = 0; i < s.size();) {
        unsigned char c = (unsigned char)s[i];
        uint32_t cp;
        int n;
        if (c < 0x80) cp = c, n = 1;
        else if ((c >> 5) == 6) cp = c & 0x1f, n = 2;
        else if ((c >> 4) == 14) cp = c & 0x0f, n = 3;
        else cp = c & 0x07, n = 4;
        for (int k = 1; k < n && i + k < s.size(); k++) cp = (cp << 6) | ((unsigned char)s[i + k] & 0x3f);
        out.push_back(cp);
        i += n;
    }
    return out;
}

inline std::string utf8_encode(uint32_t cp) {
    std::string s;
    if (cp < 0x80) s += (char)cp;
    else if (cp < 0x800) s += (char)(0xc0 | (cp >> 6)), s += (char)(0x80 | (cp & 0x3f));
    else if (cp < 0x10000) s += (char)(0xe0 | (cp >> 12)), s += (char)(0x80 | ((cp >> 6) & 0x3f)), s += (char)(0x80 | (cp & 0x3f));
    else s += (char)(0xf0 | (cp >> 18)), s += (char)(0x80 | ((cp >> 12) & 0x3f)), s += (char)(0x80 | ((cp >> 6) & 0x3f)), s += (char)(0x80 | (cp & 0x3f));
    return s;
}

// DIR/<file stem>.png: Path::new(img).with_extension("png").file_name() under DIR, as the reference's --verify names it
inline std::string verify_path(const std::string &dir, const std::string &img) {
    std::string name = img.substr(img.find_last_of('/') == std::string::npos ? 0 : img.find_last_of('/') + 1);
    const size_t dot = name.find_last_of('.');
    if (dot != std::string::npos && dot != 0) name = name.substr(0, dot);
    return dir + (dir.empty() || dir.back() == '/' ? "" : "/") + name + ".png";
}

}  // namespace cli
