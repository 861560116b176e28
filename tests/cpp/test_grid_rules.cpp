// The rules of csrc/grid_rules.h, evaluated for tests/test_grid_rules_cpu.py: a stand-alone host program that includes
// nothing of the library but that header.  It reads one request per line from stdin and answers each with one line:
//   F <bits>                                floor_int of the float with these bits (hex)
//   C <vs> <o0> <o1> <o2> <p> <axis>        cell_of (floats as hex bits)
//   I <res> <x> <y> <z>                     cube_inside and cube_index
//   B <res> <b0> .. <b5>                    box_of_bounds: x0 y0 z0 ex ey ez count, then cube_index of box_voxel(t), t = 0..count
//   O <p> <thres>                           occupied (floats as hex bits)
//   K <m> <3m ints>                         the keys of the searches that follow (answers with m)
//   Q <x> <y> <z>                           keys3_lower and keys3_upper
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "grid_rules.h"

static float from_bits(const std::string& hex) {
    const uint32_t u = (uint32_t)std::stoul(hex, nullptr, 16);
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}

int main() {
    std::vector<int32_t> keys;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char op = 0;
        in >> op;
        std::string a, b;
        if (op == 'F') {
            in >> a;
            std::printf("%d\n", mi::floor_int(from_bits(a)));
        } else if (op == 'C') {
            mi::GridFrame f;
            std::string w[5];
            int axis;
            in >> w[0] >> w[1] >> w[2] >> w[3] >> w[4] >> axis;
            f.vs = from_bits(w[0]);
            for (int k = 0; k < 3; ++k) f.origin[k] = from_bits(w[1 + k]);
            std::printf("%d\n", mi::cell_of(f, from_bits(w[4]), axis));
        } else if (op == 'I') {
            int res, x, y, z;
            in >> res >> x >> y >> z;
            const bool inside = mi::cube_inside(res, x, y, z);
            std::printf("%d %lld\n", inside ? 1 : 0, inside ? (long long)mi::cube_index(res, x, y, z) : -1ll);
        } else if (op == 'B') {
            int res, bd[6];
            in >> res;
            for (int k = 0; k < 6; ++k) in >> bd[k];
            const mi::GridBox box = mi::box_of_bounds(bd);
            std::printf("%d %d %d %d %d %d %lld", box.x0, box.y0, box.z0, box.ex, box.ey, box.ez, (long long)box.count);
            for (int64_t t = 0; t < box.count; ++t) {
                int x, y, z;
                mi::box_voxel(box, t, &x, &y, &z);
                std::printf(" %lld", mi::cube_inside(res, x, y, z) ? (long long)mi::cube_index(res, x, y, z) : -1ll);
            }
            std::printf("\n");
        } else if (op == 'O') {
            in >> a >> b;
            std::printf("%d\n", mi::occupied(from_bits(a), from_bits(b)) ? 1 : 0);
        } else if (op == 'K') {
            size_t m;
            in >> m;
            keys.assign(m * 3, 0);
            for (int32_t& k : keys) in >> k;
            std::printf("%zu\n", m);
        } else if (op == 'Q') {
            int32_t x, y, z;
            in >> x >> y >> z;
            const int64_t m = (int64_t)(keys.size() / 3);
            std::printf("%lld %lld\n", (long long)mi::keys3_lower(keys.data(), m, x, y, z),
                        (long long)mi::keys3_upper(keys.data(), m, x, y, z));
        } else if (op != 0) {
            std::printf("bad request %c\n", op);
            return 1;
        }
        if (!in) {
            std::printf("bad arguments in: %s\n", line.c_str());
            return 1;
        }
    }
    return 0;
}
