// The library dialect with character classes (include/vlg_hip.h: vlg_parse_class_query): s0.{a,b}?s1... where a position of a
// sub-pattern is a byte, an escaped byte `\x` or a class `[...]`.  Plain C++ on the host, no device: also compiled by itself.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace vlg {

struct ByteSet {                                       // 256 bits, bit c = byte c
    uint8_t w[32];
    ByteSet() { memset(w, 0, sizeof w); }
    void add(uint32_t c) { w[c >> 3] |= (uint8_t)(1u << (c & 7)); }
    bool has(uint32_t c) const { return (w[c >> 3] >> (c & 7)) & 1u; }
    uint32_t count() const { uint32_t n = 0; for (uint32_t c = 0; c < 256; ++c) n += has(c); return n; }
    uint32_t lowest() const { for (uint32_t c = 0; c < 256; ++c) if (has(c)) return c; return 256; }
};
inline uint32_t byteset_count(const uint8_t* row) { uint32_t n = 0; for (int i = 0; i < 32; ++i) n += (uint32_t)__builtin_popcount(row[i]); return n; }
inline uint32_t byteset_lowest(const uint8_t* row) { for (uint32_t c = 0; c < 256; ++c) if ((row[c >> 3] >> (c & 7)) & 1u) return c; return 256; }

struct ClassParsed {
    std::vector<ByteSet> pos;                                  // every position of the query, sub-pattern after sub-pattern
    std::vector<std::pair<uint64_t, uint64_t>> sub;            // (first position, positions)
    std::vector<uint64_t> lo, hi;                              // per sub-pattern (entry 0 unused), start to start
    uint64_t end_len = 0;
};

// status codes as in vlg_hip.h: 0 ok, 1 invalid, 4 parse
enum { kClassOk = 0, kClassInvalid = 1, kClassParse = 4 };

namespace class_detail {
// std::stoull on [s,e): optional blanks, optional sign, digits; trailing characters ignored (queries.cpp: parse_u64)
inline bool number(const char* s, const char* e, uint64_t& out)
{
    while (s < e && (*s == ' ' || (*s >= 9 && *s <= 13))) ++s;
    bool neg = false;
    if (s < e && (*s == '+' || *s == '-')) { neg = *s == '-'; ++s; }
    if (s >= e || *s < '0' || *s > '9') return false;
    uint64_t v = 0;
    while (s < e && *s >= '0' && *s <= '9') {
        const uint64_t d = (uint64_t)(*s - '0');
        if (v > (0xFFFFFFFFFFFFFFFFull - d) / 10) return false;
        v = v * 10 + d;
        ++s;
    }
    out = neg ? (uint64_t)(0 - v) : v;
    return true;
}
}  // namespace class_detail

// The query is tokenised left to right: `\x` is the byte x, `[` opens a class (closed by the next unescaped `]`), `.{` outside a
// class opens a gap `.{a,b}?` with the rules and errors of the library dialect, anything else is itself.
inline int parse_class_query(const char* re, uint64_t len, uint32_t max_sub, ClassParsed& out, std::string& why)
{
    const uint8_t* s = reinterpret_cast<const uint8_t*>(re);
    std::vector<uint64_t> raw_lo(1, 0), raw_hi(1, 0);
    uint64_t first = 0;                                        // first position of the sub-pattern in work
    uint64_t i = 0;
    while (i < len) {
        const uint8_t c = s[i];
        if (c == '\\') {
            if (i + 1 >= len) { why = "a lone '\\' at the end of the query"; return kClassParse; }
            ByteSet b; b.add(s[i + 1]);
            out.pos.push_back(b);
            i += 2;
        } else if (c == '[') {
            uint64_t j = i + 1;
            bool complement = false;
            if (j < len && s[j] == '^') { complement = true; ++j; }
            ByteSet b;
            bool closed = false, any = false;
            while (j < len) {
                if (s[j] == ']') { closed = true; ++j; break; }
                uint32_t x = s[j];
                if (x == '\\') {
                    if (j + 1 >= len) { why = "a lone '\\' at the end of the query"; return kClassParse; }
                    x = s[j + 1];
                    ++j;
                }
                ++j;
                uint32_t y = x;
                if (j + 1 < len && s[j] == '-' && s[j + 1] != ']') {                  // a range x-y ('-' in front of ']' is itself)
                    y = s[j + 1];
                    j += 2;
                    if (y == '\\') {
                        if (j >= len) { why = "a lone '\\' at the end of the query"; return kClassParse; }
                        y = s[j];
                        ++j;
                    }
                    if (x > y) { why = "class range with its ends the wrong way round"; return kClassParse; }
                }
                if (x == 0) { why = "a class holds the 0 byte"; return kClassInvalid; }
                for (uint32_t v = x; v <= y; ++v) b.add(v);
                any = true;
            }
            if (!closed) { why = "unterminated class"; return kClassParse; }
            if (!any) { why = "empty class"; return kClassParse; }
            if (complement) {
                ByteSet inv;
                for (uint32_t v = 1; v < 256; ++v) if (!b.has(v)) inv.add(v);
                b = inv;
                if (!b.count()) { why = "a complemented class that accepts no byte"; return kClassInvalid; }
            }
            out.pos.push_back(b);
            i = j;
        } else if (c == '.' && i + 1 < len && s[i + 1] == '{') {
            if (out.sub.size() + 1 >= max_sub) { why = "too many sub-patterns"; return kClassInvalid; }
            uint64_t ge = ~0ull, comma = ~0ull;
            for (uint64_t t = i; t < len; ++t) if (s[t] == '}') { ge = t; break; }
            if (ge == ~0ull) { why = "invalid gap description"; return kClassParse; }
            for (uint64_t t = i; t <= ge; ++t) if (s[t] == ',') { comma = t; break; }
            uint64_t a = 0, b = 0;
            if (comma == ~0ull || !class_detail::number(re + i + 2, re + comma, a) || !class_detail::number(re + comma + 1, re + ge, b)) {
                why = "invalid gap description";
                return kClassParse;
            }
            if (a > b) { why = "invalid gap description: min-gap > max-gap"; return kClassParse; }
            if (b >= (1ull << 62)) { why = "gap bound too large (>= 2^62)"; return kClassInvalid; }
            if (ge + 1 == len || s[ge + 1] != '?') { why = "invalid gap description: expected '?' (lazy semantics)"; return kClassParse; }
            out.sub.emplace_back(first, out.pos.size() - first);
            raw_lo.push_back(a);
            raw_hi.push_back(b);
            first = out.pos.size();
            i = ge + 2;
        } else {
            ByteSet b; b.add(c);
            out.pos.push_back(b);
            ++i;
        }
    }
    out.sub.emplace_back(first, out.pos.size() - first);
    for (auto& sp : out.sub) if (sp.second == 0) { why = "empty sub-pattern"; return kClassInvalid; }
    const size_t k = out.sub.size();
    out.lo.assign(k, 0);
    out.hi.assign(k, 0);
    for (size_t t = 1; t < k; ++t) {                           // gaps count from start to start, in positions
        out.lo[t] = raw_lo[t] + out.sub[t - 1].second;
        out.hi[t] = raw_hi[t] + out.sub[t - 1].second;
    }
    out.end_len = out.sub[k - 1].second;
    return kClassOk;
}

}  // namespace vlg
