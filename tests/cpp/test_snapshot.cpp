// The table snapshot through the C++ host mirror (worldql_server_amd/cpp/world_map.hpp):
// WorldMap::export_ops and AreaMap::subscriptions_of against hand-written expectations, then a
// restore into a second map. Built and run by tests/test_gpu_snapshot.py (needs a gfx950 GPU; exit
// code 0 = pass).
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "world_map.hpp"

using namespace worldql;

static int g_fail = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                  \
        }                                                              \
    } while (0)

struct Row {
    uint32_t world, peer;
    int64_t x, y, z;
};

static bool same(const std::vector<wq_op>& got, const std::vector<Row>& want) {
    if (got.size() != want.size()) return false;
    for (size_t i = 0; i < got.size(); ++i) {
        wq_op e;
        std::memset(&e, 0, sizeof(e));  // the padding bytes are zero too
        e.world = want[i].world;
        e.peer = want[i].peer;
        e.kind = WQ_OP_SUBSCRIBE;
        e.key_is_raw = 1;
        e.u.key[0] = want[i].x, e.u.key[1] = want[i].y, e.u.key[2] = want[i].z;
        if (std::memcmp(&got[i], &e, sizeof(e)) != 0) return false;
    }
    return true;
}

static bool same_cubes(const std::vector<CubeArea>& got, const std::vector<CubeArea>& want) {
    if (got.size() != want.size()) return false;
    for (size_t i = 0; i < got.size(); ++i)
        if (got[i].x != want[i].x || got[i].y != want[i].y || got[i].z != want[i].z) return false;
    return true;
}

int main() {
    try {
        WorldMap wm(16);
        CHECK(wm.export_ops().empty());
        AreaMap& a = wm.get_mut("alpha");  // world 0
        AreaMap& b = wm.get_mut("beta");   // world 1
        CHECK(a.subscriptions_of(7).empty());
        a.add_subscription(7, CubeArea{16, -32, 0});
        a.add_subscription(3, CubeArea{16, -32, 0});
        a.add_subscription(7, Vector3{1.0, 1.0, 1.0});      // -> (16, 16, 16)
        a.add_subscription(7, CubeArea{-48, 0, 0});
        a.add_subscription(7, CubeArea{5, 5, 5});           // off grid
        b.add_subscription(7, CubeArea{0, 0, 0});
        b.add_subscription(9, Vector3{-1.0, 20.0, 0.5});    // -> (-16, 32, 16)
        a.add_subscription(4, CubeArea{64, 0, 0});
        a.remove_subscription(4, CubeArea{64, 0, 0});       // an emptied cube yields nothing
        const std::vector<Row> all = {{0, 7, -48, 0, 0},  {0, 7, 5, 5, 5},  {0, 3, 16, -32, 0}, {0, 7, 16, -32, 0},
                                      {0, 7, 16, 16, 16}, {1, 9, -16, 32, 16}, {1, 7, 0, 0, 0}};
        CHECK(same(wm.export_ops(), all));
        wq_export_filter f{1, 0, nullptr};
        CHECK(same(wm.export_ops(&f), {{1, 9, -16, 32, 16}, {1, 7, 0, 0, 0}}));
        const uint32_t ids[] = {9, 3, 3, 1000};
        f = wq_export_filter{WQ_WORLD_INVALID, 4, ids};
        CHECK(same(wm.export_ops(&f), {{0, 3, 16, -32, 0}, {1, 9, -16, 32, 16}}));
        f = wq_export_filter{0, 4, ids};
        CHECK(same(wm.export_ops(&f), {{0, 3, 16, -32, 0}}));
        f = wq_export_filter{0, 0, ids};
        CHECK(wm.export_ops(&f).empty());
        CHECK(same_cubes(a.subscriptions_of(7), {{-48, 0, 0}, {5, 5, 5}, {16, -32, 0}, {16, 16, 16}}));
        CHECK(same_cubes(b.subscriptions_of(7), {{0, 0, 0}}));
        CHECK(b.subscriptions_of(3).empty());

        // restore: the same worlds in id order, the rows through the ordinary apply
        WorldMap again(16);
        for (const std::string& name : wm.world_names()) again.get_mut(name);
        again.apply_ops(wm.export_ops());
        CHECK(same(again.export_ops(), all));
        CHECK(again.get("beta") && again.get("beta")->world_id() == 1);
        CHECK(again.get("alpha")->is_peer_subscribed(7, Vector3{1.0, 1.0, 1.0}));
        CHECK(!again.get("alpha")->is_peer_subscribed(4, CubeArea{64, 0, 0}));
        CHECK(same_cubes(again.get("alpha")->subscriptions_of(7), a.subscriptions_of(7)));
        wm.remove_peer(7);
        CHECK(same(wm.export_ops(), {{0, 3, 16, -32, 0}, {1, 9, -16, 32, 16}}));
        CHECK(same(again.export_ops(), all));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}
