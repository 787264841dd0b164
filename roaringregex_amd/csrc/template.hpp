// template.hpp — the replacement template of regexp_replace with group references (rrx_template): its segments as the parser
// leaves them.  Pure host code without a device header: template.cpp is all there is behind it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace rrx {

constexpr size_t kTemplateSegments = 32;         // (device.hpp: kTemplateMaxSegments, what the kernels' LDS copy holds)

// One segment: a literal (ref == -1: bytes [lit_off, lit_off + lit_len) of ReplaceTemplate::lits) or a reference (ref = 0 ... 9,
// 0 the whole match).
struct TemplateSegment {
    int ref = -1;
    uint32_t lit_off = 0, lit_len = 0;
};
struct ReplaceTemplate {
    std::vector<TemplateSegment> segs;           // adjacent literals merged: no two literals side by side, none empty
    std::string lits;                            // the literals' bytes, one behind the other
    std::vector<int> refs;                       // the distinct referenced groups >= 1, ascending: the r-th is PLANE r
    int plane_of(int group) const;               // -1: not referenced
};

enum class TemplateError { none, syntax, too_many_segments };
// Bytes are literal except '\': \0 ... \9 a reference (one digit: \12 is group 1 and a literal 2), \\ one backslash; any other byte
// behind '\' and a trailing '\' are errors (syntax, *at = the offset of that '\').  More than kTemplateSegments segments:
// too_many_segments.  The empty template is valid: no segment.
TemplateError parse_template(const uint8_t *rep, size_t rep_len, ReplaceTemplate &out, size_t *at);

}  // namespace rrx
