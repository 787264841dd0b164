// template.cpp — the parser of replacement templates (template.hpp): plain host code, no device call, no handle.
#include "template.hpp"

#include <algorithm>

namespace rrx {

int ReplaceTemplate::plane_of(int group) const {
    const auto it = std::lower_bound(refs.begin(), refs.end(), group);
    return it != refs.end() && *it == group ? (int)(it - refs.begin()) : -1;
}

TemplateError parse_template(const uint8_t *rep, size_t rep_len, ReplaceTemplate &out, size_t *at) {
    out = ReplaceTemplate();
    auto literal = [&](uint8_t c) {                      // one more literal byte: into the literal in front of it, if there is one
        if (out.segs.empty() || out.segs.back().ref >= 0) {
            TemplateSegment s;
            s.lit_off = (uint32_t)out.lits.size();
            out.segs.push_back(s);
        }
        out.segs.back().lit_len++;
        out.lits.push_back((char)c);
    };
    for (size_t p = 0; p < rep_len; p++) {
        if (rep[p] != '\\') { literal(rep[p]); continue; }
        if (p + 1 == rep_len) { *at = p; return TemplateError::syntax; }
        const uint8_t c = rep[p + 1];
        if (c == '\\') literal('\\');
        else if (c >= '0' && c <= '9') {
            TemplateSegment s;
            s.ref = c - '0';
            out.segs.push_back(s);
            if (s.ref) out.refs.push_back(s.ref);
        } else { *at = p; return TemplateError::syntax; }
        p++;
    }
    if (out.segs.size() > kTemplateSegments) return TemplateError::too_many_segments;
    std::sort(out.refs.begin(), out.refs.end());
    out.refs.erase(std::unique(out.refs.begin(), out.refs.end()), out.refs.end());
    return TemplateError::none;
}

}  // namespace rrx
